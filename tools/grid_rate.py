"""Rates of the distribution grid's power flow on the device (ev2g_grid_run: a one-step launch of the step kernel, then the grid kernel, T
times per episode) next to the same one-launch-per-step run without the grid, episodes alternating between the two, one JSON line per workload.

  python tools/grid_rate.py [--workloads bus34,bus123] [--episodes 3] [--state] [--rollout]
      env-steps/s from HIP-event kernel time (last_step_n_kernel_ms), and solve_numpy's env-steps/s on one CPU core for the same node powers
      --state adds ev2g_grid_run_observed (the V2G_grid_state rows, float64 and float32, after every step) to the alternation, --rollout
      ev2g_grid_rollout under a seeded Dg -> 64 -> 64 -> P bf16 actor (whose actions differ from the all-ones block of the other runs: its
      figure is the chain's cost, not a like-for-like rate)
  rocprofv3 --kernel-trace --stats -d OUT/bus34 -- python tools/grid_rate.py --workloads bus34 --episodes 1 --no-cpu
      the grid kernel's share of a step's kernel time is rocprofv3's own statistics table

Workloads: the reference's 34-bus feeder under 4096 envs of 33 one-port chargers on 33 transformers, and its 123-bus feeder under 1024 envs of
122 chargers on 122 transformers (one transformer per non-slack bus); the network files are the test fixtures'.  The base profiles are seeded:
the nominal bus loads scaled by a factor in 0.5 .. 1.5 per scenario, step and bus, PV up to 30 % of them.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ev2gym_amd import _abi  # noqa: E402
from ev2gym_amd.grid import GridNetwork, solve_numpy  # noqa: E402
from ev2gym_amd.scenario_gen import GenConfig  # noqa: E402

KINDS = ("V2G_profitmaxV2", "V2G_profit_max")
WORKLOADS = {"bus34": (34, 4096), "bus123": (123, 1024)}


def rates(workload, episodes, net_dir, cpu, state=False, rollout=False):
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.scenario_gen import generate_native
    n_bus, E = WORKLOADS[workload]
    n = n_bus - 1
    net = GridNetwork.from_files(os.path.join(net_dir, f"Nodes_{n_bus}.csv"), os.path.join(net_dir, f"Lines_{n_bus}.csv"))
    eng = Engine(generate_native(GenConfig.v2g_profit_plus_loads(E, n, n, seed=1234)), _abi.REWARD_KINDS[KINDS[0]], _abi.STATE_KINDS[KINDS[1]],
                 flags=_abi.FLAG_LOG_SOC)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    rng = np.random.default_rng(7)
    load = np.round(net.p_values * rng.uniform(0.5, 1.5, (eng.M, T + 1, n_bus)), 1)
    p_base, q_base = net.base_profiles(load, np.round(load * rng.uniform(0.0, 0.3, load.shape), 1))
    g = eng.grid_create(net, (p_base, q_base))
    obs, rew = eng.empty((E, D)), eng.empty((E,))
    done, mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    acts, vm = eng.empty((E, P)).upload(np.ones((E, P))), eng.empty((E, n_bus))
    runs = (lambda: eng.step_n(T, acts, 0, obs, 0, rew, 0, done, 0, mask, 0, auto_reset=0, persistent=False),
            lambda: eng.grid_run(g, T, None, acts, 0, obs, 0, rew, 0, done, 0, mask, 0, vm, 0, 1.0, 50000.0))
    names = ["plain", "grid"]
    if state or rollout:
        import datetime
        from ev2gym_amd.grid import time_features
        Dg = eng.grid_state_attach(g, time_features(datetime.datetime(2022, 1, 17, 5, 0), eng.batch.timescale, T))
    if state:
        gobs, gobs32 = eng.empty((E, Dg)), eng.empty((E, Dg), np.float32)
        runs += (lambda: eng.grid_run_observed(g, T, None, acts, 0, obs, 0, rew, 0, done, 0, mask, 0, vm, 0, 1.0, 50000.0, gobs, 0, gobs32, 0),)
        names.append("observed")
    if rollout:
        from ev2gym_amd.actor import init_mlp_weights
        mlp = eng.mlp_create(*init_mlp_weights(Dg, P, seed=9, h1=64, h2=64), out_lo=-1.0, precision="bf16")

        def policy_loop():
            eng.grid_observe(g)
            eng.grid_rollout(g, mlp, T, rew, 0, done, 0, mask, 0, vm, 0, 1.0, 50000.0)
        runs += (policy_loop,)
        names.append("rollout")
    ms = tuple([] for _ in runs)
    for i in range(episodes + 1):   # the first episode of each warms up
        for which, run in enumerate(runs):
            eng.reset()
            run()
            if i:
                ms[which].append(eng.last_step_n_kernel_ms())
    eng.check_faults()
    # iteration counts of the last step's rows, and the CPU figure on that step's node powers
    it = eng.empty((E,), np.int32)
    scn = (np.arange(E) + eng.scenario_offset) % eng.M
    rows = min(E, 256)
    tr_host = np.array([eng.peek(e)["tr_power"] for e in range(rows)])
    P_last, Q_last = p_base[scn[:rows], T - 1] + tr_host, q_base[scn[:rows], T - 1]
    dp, dq = eng.empty((rows, n)).upload(P_last), eng.empty((rows, n)).upload(Q_last)
    eng.grid_solve(g, dp, dq, rows, None, None, it, None)
    eng.synchronize()
    iters = it.to_host()[:rows]
    cpu_rate = None
    if cpu:
        t0 = time.perf_counter()
        ref = solve_numpy(net.K, net.L, P_last, Q_last, net.s_base)
        cpu_rate = round(rows / (time.perf_counter() - t0))
        assert np.abs(ref["iters"] - iters).max() <= 1   # (unguarded rows: a residual at the tolerance may fall on either side)
    rate = lambda m: round(E * T / (m / 1e3))   # noqa: E731
    plain, grid = statistics.median(ms[0]), statistics.median(ms[1])
    print(json.dumps(dict(workload=workload, n_bus=n_bus, envs=E, ports=P, transformers=eng.R, steps=T, step_kernel=eng.kernel_name,
                          plain_env_steps_per_s=rate(plain), plain_range=[rate(max(ms[0])), rate(min(ms[0]))],
                          grid_env_steps_per_s=rate(grid), grid_range=[rate(max(ms[1])), rate(min(ms[1]))],
                          plain_us_per_step=round(plain * 1e3 / T, 3), grid_us_per_step=round(grid * 1e3 / T, 3),
                          grid_over_plain=round(grid / plain, 4), iterations_mean=round(float(iters.mean()), 2),
                          iterations_range=[int(iters.min()), int(iters.max())], solve_numpy_env_steps_per_s_one_core=cpu_rate,
                          **{f"{nm}_{k}": v for nm, m in zip(names[2:], ms[2:]) for k, v in
                             (("env_steps_per_s", rate(statistics.median(m))), ("range", [rate(max(m)), rate(min(m))]),
                              ("us_per_step", round(statistics.median(m) * 1e3 / T, 3)), ("over_grid", round(statistics.median(m) / grid, 4)))},
                          grid_stats_violating_steps_mean=round(float(eng.grid_get_stats(g)["voltage_violation_counter_per_step"].mean()), 2))),
          flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="bus34,bus123")
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--network-dir", default=os.path.join(ROOT, "tests", "golden", "grid"))
    ap.add_argument("--no-cpu", action="store_true", help="skip solve_numpy's timing")
    ap.add_argument("--state", action="store_true", help="also time ev2g_grid_run_observed")
    ap.add_argument("--rollout", action="store_true", help="also time ev2g_grid_rollout")
    args = ap.parse_args()
    for w in args.workloads.split(","):
        rates(w, args.episodes, args.network_dir, not args.no_cpu, args.state, args.rollout)
