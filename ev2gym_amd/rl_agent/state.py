"""state_function plugins (mirror of the reference's ev2gym/rl_agent/state.py, same names and signature).

`f(env, *args) -> 1-D float64 array`.  The three functions below are fused into the HIP step kernel when passed
as `state_function=`; their Python bodies evaluate the same layout on the single-env facade and serve as the
host fallback / documentation of the observation layout (transformer-major over ports).
"""
import math

import numpy as np


def PublicPST(env, *args):
    """state.py:6-63   [step/T, setpoint[step] (0 at the end), usage[step-1], per port (full?, energy, time since arrival)]"""
    s = env.current_step
    state = [s / env.simulation_length,
             env.power_setpoints[s] if s < env.simulation_length else 0.0,
             env.current_power_usage[s - 1]]
    for tr in env.transformers:
        for cs in env.charging_stations:
            if cs.connected_transformer == tr.id:
                for ev in cs.evs_connected:
                    if ev is not None:
                        state += [1 if ev.get_soc() == 1 else 0.5, ev.total_energy_exchanged, s - ev.time_of_arrival]
                    else:
                        state += [0.0, 0.0, 0.0]
    return np.array(state, dtype=np.float64)


def _v2g_head(env):
    s = env.current_step
    prices = np.abs(np.asarray(env.charge_prices)[0, s:s + 20])
    if len(prices) < 20:
        prices = np.append(prices, np.zeros(20 - len(prices)))
    return [float(s), env.current_power_usage[s - 1]] + list(prices)


def _ports_of(env, tr):
    out = []
    for cs in env.charging_stations:
        if cs.connected_transformer == tr.id:
            for ev in cs.evs_connected:
                out += [ev.get_soc(), ev.time_of_departure - env.current_step] if ev is not None else [0.0, 0.0]
    return out


def V2G_profit_max(env, *args):
    """state.py:65-106"""
    state = _v2g_head(env)
    for tr in env.transformers:
        state += _ports_of(env, tr)
    return np.array(state, dtype=np.float64)


def V2G_profit_max_loads(env, *args):
    """state.py:108-155"""
    state = _v2g_head(env)
    for tr in env.transformers:
        loads, pv = tr.get_load_pv_forecast(step=env.current_step, horizon=20)
        state += list(np.asarray(loads) - np.asarray(pv))
        state += list(tr.get_power_limits(step=env.current_step, horizon=20))
        state += _ports_of(env, tr)
    return np.array(state, dtype=np.float64)


def V2G_grid_state(env, *args):
    """state.py:216-278   [weekday/7, sin(hour), cos(hour), charge price[step] (signed; 0 at the end), setpoint[step] (0 at the end),
    usage[step-1], base P and Q of every non-slack bus, per port in charger order (capacity, steps to departure + 1, the charger's bus)].
    On the device this row is built by the grid (`EV2GymVec(grid=..., state_function="V2G_grid_state")`, csrc/ev2g_grid.h); the body below
    serves an env object that simulates the grid itself and carries node_active_power / node_reactive_power [n_bus, T]."""
    if getattr(env, "node_active_power", None) is None:
        raise NotImplementedError("V2G_grid_state reads env.node_active_power / node_reactive_power: the single-env facade has no grid path; "
                                  "use EV2GymVec(grid=..., grid_profiles=..., state_function='V2G_grid_state')")
    from ..grid import grid_state_numpy
    s, T = env.current_step, env.simulation_length
    hour = env.sim_date.hour / 24 * 2 * math.pi
    col = max(s - 1, 0)
    # grid_state_numpy indexes its profile rows by step counter: only row s is read, and it is what column max(s - 1, 0) holds
    n = np.asarray(env.node_active_power).shape[0] - 1
    p, q = np.zeros((T + 1, n)), np.zeros((T + 1, n))
    p[s], q[s] = np.asarray(env.node_active_power)[1:, col], np.asarray(env.node_reactive_power)[1:, col]
    cap, dep, bus = [], [], []
    for cs in env.charging_stations:
        for ev in cs.evs_connected:
            cap.append(np.nan if ev is None else ev.current_capacity)
            dep.append(0 if ev is None else ev.time_of_departure)
            bus.append(cs.connected_bus)
    return grid_state_numpy(s, T, (env.sim_date.weekday() / 7, math.sin(hour), math.cos(hour)), np.asarray(env.charge_prices)[0],
                            env.power_setpoints, env.current_power_usage, p, q, cap, dep, bus)


V2G_profit_max_loads._ev2g_kind = 0
PublicPST._ev2g_kind = 1
V2G_profit_max._ev2g_kind = 2
