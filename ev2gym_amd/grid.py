"""The distribution grid of `simulate_grid: True` (reference: ev2gym/models/grid.py, ev2gym/models/grid_utility/grid_tensor.py): the network
matrices of the Laurent power flow, the base load profiles, and a plain numpy restatement of the iteration.

The device runs the iteration (csrc/ev2g_grid.h, `Engine.grid_create / grid_solve / grid_run`, `EV2GymVec(grid=...)`); everything here is host
preparation, done once per network, and `solve_numpy`, the CPU check of the kernel.  numpy only.  For the grid scenario's observation and
statistics (`EV2GymVec(state_function="V2G_grid_state", grid_start=, grid_statistics=True)`, `Engine.grid_state_attach / grid_observe /
grid_run_observed / grid_rollout / grid_get_stats`) it holds `time_features`, `grid_state_dim`, and the numpy restatements `grid_state_numpy`
and `voltage_statistics`.

    net = GridNetwork.from_files("Nodes_34.csv", "Lines_34.csv")
    p_base, q_base = net.base_profiles(load, pv)        # load / pv: [T + 1, n_bus] in kW, column 0 the slack bus
    env = EV2GymVec(scenarios=batch, grid=net, grid_profiles=(load, pv), grid_reward="V2G_grid_simple_reward")

The reference samples `load` from a fitted generator (data/augmentor.pkl) that its repository does not ship; here the profiles are the caller's
arrays (PowerGrid.reset's `load_data` / `pv_data` arguments, grid.py:79-91).
"""
from __future__ import annotations

import datetime
import math

import numpy as np

# reward names of the reference that are a step reward plus a voltage term, as (reward kind of the step kernel or None, base_weight, voltage_weight)
GRID_REWARDS = {
    "V2G_grid_simple_reward": (None, 0.0, 1000.0),              # rl_agent/reward.py:114-121: 1000 * loss_v
    "Grid_V2G_profitmaxV2": ("V2G_profitmaxV2", 1.0, 50000.0),  # rl_agent/reward.py:215-279: V2G_profitmaxV2's body + 50_000 * loss_v
}


def voltage_loss(vm):
    """sum_i min(0, 0.05 - |1 - vm_i|) over the last axis (rl_agent/reward.py:117-119)."""
    vm = np.asarray(vm, np.float64)
    return np.minimum(np.zeros_like(vm), 0.05 - np.abs(1 - vm)).sum(axis=-1)


def time_features(start, timescale_min, T):
    """[T + 1, 3]: weekday / 7, sin(hour / 24 * 2 pi), cos(hour / 24 * 2 pi) of sim_date at every step counter 0 .. T, the first three
    columns of V2G_grid_state (rl_agent/state.py:222-224).  sim_date starts at `start` and advances by `timescale_min` minutes per step
    (ev2gym_env.py:560); weekday and hour roll over at midnight."""
    out = np.empty((int(T) + 1, 3), np.float64)
    date = start
    for c in range(int(T) + 1):
        out[c] = (date.weekday() / 7, math.sin(date.hour / 24 * 2 * math.pi), math.cos(date.hour / 24 * 2 * math.pi))
        date = date + datetime.timedelta(minutes=timescale_min)
    return out


def grid_state_dim(n_bus, P):
    """Width of a V2G_grid_state row: 6 + 2 (n_bus - 1) + 3 P."""
    return 6 + 2 * (int(n_bus) - 1) + 3 * int(P)


def grid_state_numpy(c, T, time_row, charge_prices, power_setpoints, power_usage, p_base, q_base, port_capacity, port_departure, port_bus):
    """One V2G_grid_state row (rl_agent/state.py:216-278) from plain arrays, for step counter c of a T-step episode: time_row [3] (a row of
    time_features), charge_prices / power_setpoints [T], power_usage [T] (current_power_usage; read at c - 1, and as 0 at c == 0, where the
    reference reads the last entry of a freshly zeroed array), p_base / q_base [T + 1, n] (row c is what node_active_power /
    node_reactive_power [1:, max(c - 1, 0)] hold), and per port in reference port order the EV's current_capacity, its time_of_departure
    and the charger's bus -- a NaN capacity marks an empty port (three zeros).  Copies and integer differences only."""
    P = len(port_capacity)
    n = np.asarray(p_base).shape[1]
    row = np.zeros(6 + 2 * n + 3 * P, np.float64)
    row[0:3] = time_row
    row[3] = charge_prices[c] if c < T else 0.0
    row[4] = power_setpoints[c] if c < T else 0.0
    row[5] = power_usage[c - 1] if c > 0 else 0.0
    row[6:6 + n] = p_base[c]
    row[6 + n:6 + 2 * n] = q_base[c]
    for i in range(P):
        if not np.isnan(port_capacity[i]):
            row[6 + 2 * n + 3 * i:9 + 2 * n + 3 * i] = (port_capacity[i], int(port_departure[i]) - c + 1, port_bus[i])
    return row


def voltage_statistics(vm):
    """(voltage_violation, voltage_violation_counter, voltage_violation_counter_per_step) of get_statistics (utilities/utils.py:69-78) for
    the node voltages vm [T, n_bus] of one episode (the reference holds them as [n_bus, T]; sums and counts do not care): the sum of
    min(0, 0.05 - |1 - v|) over every entry, the number of entries below 0.95 or above 1.05, the number of steps with at least one."""
    vm = np.asarray(vm, np.float64)
    out = (vm < 0.95) | (vm > 1.05)
    return float(np.minimum(np.zeros_like(vm), 0.05 - np.abs(1 - vm)).sum()), int(np.sum(vm < 0.95) + np.sum(vm > 1.05)), int(np.sum(np.any(out, axis=-1)))


def _read_csv(path):
    return np.atleast_2d(np.genfromtxt(path, delimiter=",", skip_header=1, dtype=np.float64))


class GridNetwork:
    """Ybus of a radial feeder and the two matrices of the constant-power Laurent iteration, K = -inv(Ydd) and L = K Yds
    (grid_tensor.py:83-118, 212-283).  Bus 1 is the slack bus (the reference assumes so too, grid_tensor.py:269-278)."""

    def __init__(self, bus_info, branch_info, s_base=1000, v_base=11):
        bus, br = np.asarray(bus_info, np.float64), np.asarray(branch_info, np.float64)
        self.s_base, self.v_base = s_base, v_base
        self.n_bus = nb = bus.shape[0]
        self.p_values, self.q_values = bus[:, 2], bus[:, 3]
        self.pf = (self.q_values / (self.p_values + 1e-6))[1:]   # grid_tensor.py:85-87 (slack ignored)
        z_base = v_base ** 2 * 1000 / s_base
        stat = br[:, 5]
        Ys = stat / ((br[:, 2] + 1j * br[:, 3]) / z_base)   # series admittance
        Bc = stat * br[:, 4] * z_base                       # line charging susceptance
        tap = stat * br[:, 6]
        Ytt = Ys + 1j * Bc / 2
        Yff = Ytt / tap
        Yft = -Ys / tap
        f, t = br[:, 0].astype(int) - 1, br[:, 1].astype(int) - 1
        Y = np.zeros((nb, nb), np.complex128)
        np.add.at(Y, (f, f), Yff)
        np.add.at(Y, (f, t), Yft)
        np.add.at(Y, (t, f), Yft)
        np.add.at(Y, (t, t), Ytt)
        self.Ybus = Y
        self.K = -np.linalg.inv(Y[1:, 1:])
        self.L = (self.K @ Y[0, 1:].reshape(-1, 1)).reshape(-1)   # Yds = Ysd.T (grid_tensor.py:270-271)

    @classmethod
    def from_files(cls, bus_csv, branch_csv, s_base=1000, v_base=11):
        """bus_csv: NODES,Tb,PD,QD,...; branch_csv: FROM,TO,R,X,B,STATUS,TAP (the reference's data/network_data files)."""
        return cls(_read_csv(bus_csv), _read_csv(branch_csv), s_base=s_base, v_base=v_base)

    def base_profiles(self, load_data, pv_data):
        """P_base = load[:, 1:] - pv[:, 1:] and Q_base = round(load[:, 1:] * pf, 1), row t being what PowerGrid holds before the EV powers of
        step t are added (grid.py:110-116, 133-139).  load_data / pv_data: [..., rows, n_bus] in kW; the inputs are not modified."""
        load, pv = np.asarray(load_data, np.float64), np.asarray(pv_data, np.float64)
        if load.shape != pv.shape or load.shape[-1] != self.n_bus:
            raise ValueError(f"base_profiles: load {load.shape} / pv {pv.shape} must be equal and end in n_bus = {self.n_bus}")
        active = load[..., 1:].copy()
        reactive = (active * self.pf).round(1)
        active -= pv[..., 1:]
        return active, reactive

    def solve_numpy(self, p_kw, q_kw, tolerance=1e-6, max_iter=100, residuals=False):
        return solve_numpy(self.K, self.L, p_kw, q_kw, self.s_base, tolerance, max_iter, residuals)


def solve_numpy(K, L, p_kw, q_kw, s_base=1000, tolerance=1e-6, max_iter=100, residuals=False):
    """The reference's iteration (grid.py:151-199 with ts = 1, through run_pf_tensor's scaling, grid_tensor.py:594-598) for every row of
    p_kw / q_kw [rows, n] on its own: {"v": [rows, n] complex, "vm": [rows, n + 1] with the slack's 1.0 in front, "iters": [rows],
    "loss_v": [rows]} and, with residuals=True, "res": [rows, 2] the last two values of tol (inf where there was none)."""
    K = np.asarray(K, np.complex128)
    L = np.asarray(L, np.complex128).reshape(-1, 1)
    P, Q = np.atleast_2d(np.asarray(p_kw, np.float64)), np.atleast_2d(np.asarray(q_kw, np.float64))
    rows, n = P.shape
    v_out, it_out, res = np.empty((rows, n), np.complex128), np.zeros(rows, np.int32), np.full((rows, 2), np.inf)
    for r in range(rows):
        S = (P[r] / s_base + 1j * (Q[r] / s_base)).reshape(-1, 1)
        v0 = np.ones((n, 1)) + 1j * np.zeros((n, 1))
        it, tol = 0, np.inf
        while it < max_iter and tol >= tolerance:
            lam = np.conj(S * (1 / v0))
            vk = K @ lam + L
            tol = np.max(np.abs(np.abs(vk) - np.abs(v0)))
            res[r] = res[r, 1], tol
            v0 = vk
            it += 1
        v_out[r], it_out[r] = v0[:, 0], it
    vm = np.concatenate([np.ones((rows, 1)), np.abs(v_out)], axis=1)
    out = {"v": v_out, "vm": vm, "iters": it_out, "loss_v": voltage_loss(vm)}
    if residuals:
        out["res"] = res
    return out
