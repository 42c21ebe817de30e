"""CPU side of V2G_grid_state and the grid statistics (ev2gym_amd/grid.py, csrc/ev2g_grid.h, ev2g_grid_state_* / _observe / _run_observed /
_rollout / _get_stats): the numpy restatement of the row and the time features against rows the reference's own V2G_grid_state returned
(tests/golden/grid/grid_state.npz, recorded by tools/capture_grid_state_fixtures.py), the voltage statistics on a hand-made matrix, the
refusals that come before any device call, the C-ABI surface."""
import ctypes
import datetime
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from tests.test_grid_cpu import GRID_DIR, network

STATE_SYMBOLS = ("ev2g_grid_state_attach", "ev2g_grid_state_dim", "ev2g_grid_observe", "ev2g_grid_run_observed", "ev2g_grid_rollout",
                 "ev2g_grid_get_stats")


def state_fixture():
    return np.load(os.path.join(GRID_DIR, "grid_state.npz"))


def test_grid_state_numpy_and_time_features_reproduce_the_reference_rows_bit_for_bit():
    """Every row of every recorded episode: step counters 0 .. T, an episode from Sunday 22:00 in hour steps (midnight and the week roll
    over), negative prices, empty and occupied ports on one- to three-port chargers."""
    from ev2gym_amd.grid import grid_state_dim, grid_state_numpy, time_features
    z = state_fixture()
    assert os.path.getsize(os.path.join(GRID_DIR, "grid_state.npz")) < 1 << 20
    n_eps, T1, Dg = z["rows"].shape
    T, P, n = T1 - 1, int(z["cs_ports"].sum()), int(z["n_bus"]) - 1
    assert Dg == grid_state_dim(int(z["n_bus"]), P) == 6 + 2 * n + 3 * P and z["cs_ports"].max() > 1
    bus = np.repeat(z["cs_bus"], z["cs_ports"])
    seen = dict(empty=0, occupied=0, weekdays=set(), negative_price=False)
    for k in range(n_eps):
        tf = time_features(datetime.datetime(*(int(x) for x in z["start"][k])), int(z["timescale"][k]), T)
        assert tf.shape == (T + 1, 3) and np.array_equal(tf, z["rows"][k][:, :3]), k
        seen["weekdays"].update(tf[:, 0].tolist())
        for c in range(T + 1):
            here = (z["ev_arrival"][k] <= c) & (c <= z["ev_departure"][k])
            cap = np.where(here, z["ev_capacity"][k, c], np.nan)
            row = grid_state_numpy(c, T, tf[c], z["prices"][k], z["setpoints"][k], z["usage"][k], z["p_base"][k], z["q_base"][k], cap,
                                   z["ev_departure"][k], bus)
            assert row.dtype == np.float64 and np.array_equal(row, z["rows"][k, c]), (k, c)
            seen["empty"] += int((~here).sum())
            seen["occupied"] += int(here.sum())
            seen["negative_price"] |= bool(row[3] < 0)
        assert z["rows"][k, 0, 5] == 0.0 and z["rows"][k, T, 3] == 0.0 and z["rows"][k, T, 4] == 0.0
    assert seen["empty"] and seen["occupied"] and seen["negative_price"] and len(seen["weekdays"]) >= 3
    # the Sunday-night episode: weekday 6 -> 0 and hour 23 -> 0 between two rows
    tf = time_features(datetime.datetime(2022, 1, 16, 22, 0), 60, 3)
    assert tf[1, 0] == 6 / 7 and tf[2, 0] == 0.0 and tf[2, 1] == 0.0 and tf[2, 2] == 1.0


def test_voltage_statistics_on_a_hand_made_matrix():
    from ev2gym_amd.grid import voltage_statistics
    vm = np.ones((4, 5))
    vm[0, 1], vm[0, 3] = 0.94, 1.06          # two violations in step 0
    vm[2, 4] = 0.90                          # one in step 2
    vm[3, 2], vm[3, 3] = 0.95, 1.05          # on the band's edge: neither `<` nor `>` counts them
    total, count, steps = voltage_statistics(vm)
    assert (count, steps) == (3, 2)
    want = (0.05 - abs(1 - 0.94)) + (0.05 - abs(1 - 1.06)) + (0.05 - abs(1 - 0.90))
    assert want < 0 and abs(total - want) <= 1e-15
    assert voltage_statistics(np.ones((3, 4))) == (0.0, 0, 0)


def test_refusals_before_any_device_call():
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.scenario_gen import GenConfig, generate
    from ev2gym_amd.vec_env import EV2GymVec, grid_state_setup
    from ev2gym_amd.rl_agent.state import V2G_grid_state
    batch = generate(GenConfig.v2g_profit_plus_loads(2, 4, 1, seed=3, simulation_length=8))
    for fn in ("V2G_grid_state", V2G_grid_state):
        with pytest.raises(ValueError, match="only together with grid="):
            EV2GymVec(scenarios=batch, state_function=fn, reward_function="profit_maximization", use_torch=False)
    net, day = network(34), datetime.datetime(2022, 1, 17, 5, 0)
    with pytest.raises(ValueError, match="list of 5 datetimes"):
        grid_state_setup("V2G_grid_state", net, [day] * 4, M=5, T=8, timescale=15)
    with pytest.raises(ValueError, match="list of 5 datetimes"):
        grid_state_setup("V2G_grid_state", net, None, M=5, T=8, timescale=15)
    with pytest.raises(ValueError, match="grid_start is the starting date"):
        grid_state_setup("PublicPST", net, day, M=5, T=8, timescale=15)
    assert grid_state_setup("PublicPST", None, None, M=5, T=8, timescale=15) is None
    assert grid_state_setup("V2G_grid_state", net, day, M=5, T=8, timescale=15).shape == (9, 3)
    assert grid_state_setup(V2G_grid_state, net, [day] * 5, M=5, T=8, timescale=15).shape == (5, 9, 3)
    eng = Engine.__new__(Engine)
    eng._h, eng.M, eng.T = None, 5, 8
    for shape in ((8, 3), (9, 2), (4, 9, 3), (5, 9, 3, 1)):
        with pytest.raises(ValueError, match="time_features has shape"):
            eng.grid_state_attach(None, np.zeros(shape))
    # the facade has no grid path: the plugin says so
    import types
    with pytest.raises(NotImplementedError, match="no grid path"):
        V2G_grid_state(types.SimpleNamespace(current_step=0))


def test_the_plugin_body_reproduces_the_reference_rows_on_an_env_with_node_powers():
    """The plugin of the reference's name on a duck-typed env laid out as the reference's (node powers [n_bus, T], column max(c - 1, 0))."""
    import types
    from ev2gym_amd.rl_agent.state import V2G_grid_state
    z = state_fixture()
    T, k, n_bus = z["rows"].shape[1] - 1, 1, int(z["n_bus"])
    for c in (0, 4, T):
        env = types.SimpleNamespace(current_step=c, simulation_length=T, power_setpoints=z["setpoints"][k], charge_prices=z["prices"][k][None],
                                    current_power_usage=np.where(np.arange(T) < c, z["usage"][k], 0.0))
        env.sim_date = datetime.datetime(*(int(x) for x in z["start"][k])) + c * datetime.timedelta(minutes=int(z["timescale"][k]))
        env.node_active_power, env.node_reactive_power = np.zeros((n_bus, T)), np.zeros((n_bus, T))
        env.node_active_power[1:, max(c - 1, 0)], env.node_reactive_power[1:, max(c - 1, 0)] = z["p_base"][k, c], z["q_base"][k, c]
        env.charging_stations, p = [], 0
        for n_ports, bus in zip(z["cs_ports"], z["cs_bus"]):
            evs = []
            for _ in range(n_ports):
                here = z["ev_arrival"][k, p] <= c <= z["ev_departure"][k, p]
                evs.append(types.SimpleNamespace(current_capacity=z["ev_capacity"][k, c, p], time_of_departure=int(z["ev_departure"][k, p])) if here else None)
                p += 1
            env.charging_stations.append(types.SimpleNamespace(evs_connected=evs, connected_bus=int(bus)))
        assert np.array_equal(V2G_grid_state(env), z["rows"][k, c]), c


def test_c_abi_surface():
    from ev2gym_amd import _abi, build, engine
    L = ctypes.CDLL(build.build())
    hdr = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "ev2g.h")).read()
    for name in STATE_SYMBOLS:
        assert hasattr(L, name) and name in engine.EXPORTED_SYMBOLS and name + "(" in hdr, name
    assert "V2G_grid_state" not in _abi.STATE_KINDS and _abi.ABI_VERSION == 4   # a property of a grid, not a step-kernel specialisation
