"""Records tests/golden/grid/grid_state.npz from the reference's own V2G_grid_state (rl_agent/state.py:216-278; CPU, run once where a checkout
of the reference exists, like tools/capture_grid_fixtures.py; oracle/ref_import.py makes it importable).

The reference's full env cannot be built for the grid scenario (PowerGrid.__init__ opens the load generator's pickle, which its repository
does not ship), and the state function reads a dozen attributes only: it is called on small duck-typed env objects that carry exactly those --
sim_date, charge_prices, power_setpoints, current_power_usage, node_active_power, node_reactive_power, current_step, simulation_length and
charging_stations whose evs_connected entries hold current_capacity / time_of_departure.  The env's bookkeeping around them is restated here:
sim_date advances by `timescale` minutes per step (ev2gym_env.py:560); current_power_usage is zero from the current step on; column 0 of the
node powers holds base row 0 after reset and column t holds base row t + 1 after step t (grid.py:131-141, ev2gym_env.py:395).

Per episode (seeded inputs; rows for EVERY step counter 0 .. T, so c = 0, the middle and c = T are all there):
  start [5] year, month, day, hour, minute; timescale     one episode starts at 22:00 on a Sunday with hour steps: it crosses midnight and the week
  prices, setpoints, usage [T]; p_base, q_base [T + 1, n]  prices are signed (the state does not take their abs)
  ev_arrival, ev_departure [P], ev_capacity [T + 1, P]     at most one EV per port; a port holds it while arrival <= c <= departure
  rows [T + 1, Dg]                                          what the reference returned
and for all of them the chargers' port counts (1, 2, 3, 2: multi-port chargers) and buses.  Data only.

    python tools/capture_grid_state_fixtures.py
"""
import datetime
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "grid", "grid_state.npz")
T, N_BUS = 8, 6
CS_PORTS, CS_BUS = (1, 2, 3, 2), (0, 3, 3, 4)
EPISODES = (((2022, 1, 17, 5, 0), 15), ((2022, 1, 16, 22, 0), 60), ((2023, 7, 1, 23, 30), 30))   # a Monday morning; Sunday night into Monday; Saturday night


def episode(state_fn, start, timescale, rng):
    n, P = N_BUS - 1, sum(CS_PORTS)
    prices = np.round(rng.uniform(-0.05, 0.3, T), 4)
    prices[1] = -abs(prices[1]) - 0.01   # a negative price: the sign has to survive
    setpoints = np.round(rng.uniform(0.0, 80.0, T), 3)
    usage = np.round(rng.uniform(-40.0, 90.0, T), 3)
    p_base = np.round(rng.uniform(5.0, 300.0, (T + 1, n)), 1)
    q_base = np.round(p_base * rng.uniform(0.1, 0.5, n), 1)
    arr = rng.integers(0, T, P)
    dep = np.minimum(arr + rng.integers(1, T, P), T + 2)
    arr[0], dep[0] = T + 5, T + 9   # a port that stays empty
    arr[1], dep[1] = 0, T + 1       # and one that is occupied throughout
    cap = np.round(rng.uniform(5.0, 70.0, (T + 1, P)), 3)
    rows = []
    for c in range(T + 1):
        env = types.SimpleNamespace(current_step=c, simulation_length=T)
        env.sim_date = datetime.datetime(*start) + c * datetime.timedelta(minutes=timescale)
        env.charge_prices = np.stack([prices, prices * 1.1])
        env.power_setpoints = setpoints
        env.current_power_usage = np.where(np.arange(T) < c, usage, 0.0)
        nap, nrp = np.zeros((N_BUS, T)), np.zeros((N_BUS, T))
        nap[1:, 0], nrp[1:, 0] = p_base[0], q_base[0]
        for t in range(c):
            nap[1:, t], nrp[1:, t] = p_base[t + 1], q_base[t + 1]
        nap[0], nrp[0] = 999.0, 999.0   # the slack's row is never read
        env.node_active_power, env.node_reactive_power = nap, nrp
        env.charging_stations, p = [], 0
        for n_ports, bus in zip(CS_PORTS, CS_BUS):
            evs = []
            for _ in range(n_ports):
                here = arr[p] <= c <= dep[p]
                evs.append(types.SimpleNamespace(current_capacity=cap[c, p], time_of_departure=int(dep[p])) if here else None)
                p += 1
            env.charging_stations.append(types.SimpleNamespace(evs_connected=evs, connected_bus=bus))
        rows.append(np.asarray(state_fn(env), np.float64))
    return dict(start=np.array(start), timescale=timescale, prices=prices, setpoints=setpoints, usage=usage, p_base=p_base, q_base=q_base,
                ev_arrival=arr, ev_departure=dep, ev_capacity=cap, rows=np.array(rows))


if __name__ == "__main__":
    from oracle.ref_import import import_reference
    import_reference()
    from ev2gym.rl_agent.state import V2G_grid_state
    rng = np.random.default_rng(20240611)
    eps = [episode(V2G_grid_state, start, ts, rng) for start, ts in EPISODES]
    out = {k: np.array([e[k] for e in eps]) for k in eps[0]}
    assert out["rows"].shape == (len(EPISODES), T + 1, 6 + 2 * (N_BUS - 1) + 3 * sum(CS_PORTS))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, n_bus=N_BUS, cs_ports=np.array(CS_PORTS), cs_bus=np.array(CS_BUS), **out)
    print(f"wrote {OUT}: rows {out['rows'].shape}, {os.path.getsize(OUT)} bytes")
