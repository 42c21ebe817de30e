"""Rates of the reference's env-reading heuristic agents evaluated on the device (ev2g_heuristic_run: the agent's launch, then a one-step
launch of the step kernel, T times per episode), one JSON line per (workload, agent).

  python tools/heuristic_rate.py [--workloads cfg2,cfg3,cfg4] [--episodes 3]
      env-steps/s from HIP-event kernel time (last_step_n_kernel_ms), next to the same per-step launches with fixed actions (`step_only`)
  rocprofv3 --kernel-trace --stats -d OUT/cfg2 -- python tools/heuristic_rate.py --workloads cfg2 --episodes 1
  python tools/heuristic_rate.py --workloads cfg3 --link 0.1,0.1
      ev2g_link_run (the reference's failed-command / delayed-observation models, csrc/ev2g_link.h) next to the plain per-step launches,
      episodes alternating between the two: fixed actions, and one RoundRobin run (p_delay needs a PublicPST workload: cfg3)
  python tools/heuristic_rate.py --shares OUT
      the agent kernel's share of each (agent + step) pair, from the dispatches of every kernel_trace.csv under OUT

The workloads are bench.py's shapes; cfg2 and cfg4 are drawn with power setpoints (their configs have none, and RoundRobin charges
ceil(setpoint / average charger power) EVs per step: without setpoints it never charges and its queue never rotates; the same holds
for the two RoundRobin_GF agents).
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ev2gym_amd import _abi  # noqa: E402
from ev2gym_amd.scenario_gen import GenConfig  # noqa: E402

DEFAULT = ("ProfitMax_TrPenalty_UserIncentives", "V2G_profit_max_loads")
PST = ("SquaredTrackingErrorReward", "PublicPST")
WORKLOADS = {
    "cfg2": (4096, lambda E, s: GenConfig.v2g_profit_plus_loads(E, 50, 1, seed=s, power_setpoint_enabled=True), DEFAULT),
    "cfg3": (8192, lambda E, s: GenConfig.public_pst(E, 20, seed=s), PST),
    "cfg4": (2048, lambda E, s: GenConfig.v2g_profit_plus_loads(E, 1000, 50, seed=s, power_setpoint_enabled=True), DEFAULT),
}
AGENTS = {k: n for n, k in _abi.AGENT_KINDS.items()}


def link_rates(workload, episodes, p_fail, p_delay):
    """Plain per-step launches and the same launches under a link, alternating episode by episode: env-steps/s of HIP-event kernel time."""
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.scenario_gen import generate_native
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    obs, rew = eng.empty((E, D)), eng.empty((E,))
    done, mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    acts = eng.empty((E, P)).upload(np.ones((E, P)))
    link, rr = eng.link_create(p_fail, p_delay, seed_act=1, seed_obs=2), eng.heuristic_create("RoundRobin")
    out = (None, 0, obs, 0, rew, 0, done, 0, mask, 0)
    pairs = {"fixed actions": (lambda: eng.step_n(T, acts, 0, *out[2:], auto_reset=0, persistent=False),
                               lambda: eng.link_run(link, T, None, acts, 0, *out[2:])),
             "RoundRobin": (lambda: eng.heuristic_run(rr, T, *out), lambda: eng.link_run(link, T, rr, *out))}
    for name, runs in pairs.items():
        ms = ([], [])
        for i in range(episodes + 1):   # the first episode of each warms up
            for which, run in enumerate(runs):
                eng.reset(obs)
                if which and p_delay > 0:
                    eng.link_observe(link, obs)
                run()
                if i:
                    ms[which].append(eng.last_step_n_kernel_ms())
        eng.check_faults()
        rate = lambda m: round(E * T / (m / 1e3))   # noqa: E731
        plain, linked = statistics.median(ms[0]), statistics.median(ms[1])
        print(json.dumps(dict(workload=workload, source=name, link=[p_fail, p_delay], envs=E, ports=P, steps=T, step_kernel=eng.kernel_name,
                              plain_env_steps_per_s=rate(plain), plain_range=[rate(max(ms[0])), rate(min(ms[0]))],
                              link_env_steps_per_s=rate(linked), link_range=[rate(max(ms[1])), rate(min(ms[1]))],
                              plain_us_per_step=round(plain * 1e3 / T, 3), link_us_per_step=round(linked * 1e3 / T, 3),
                              link_over_plain=round(linked / plain, 4))), flush=True)
    eng.close()


def rates(workload, episodes):
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.scenario_gen import generate_native
    E, gen, kinds = WORKLOADS[workload]
    batch = generate_native(gen(E, 1234))
    eng = Engine(batch, _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    obs, rew = eng.empty((E, D)), eng.empty((E,))
    done, mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    acts = eng.empty((E, P)).upload(np.ones((E, P)))

    def timed(run):
        ms = []
        for i in range(episodes + 1):   # the first episode warms up
            eng.reset()
            run()
            if i:
                ms.append(eng.last_step_n_kernel_ms())
        eng.check_faults()
        return statistics.median(ms), ms

    step_ms, _ = timed(lambda: eng.step_n(T, acts, 0, obs, 0, rew, 0, done, 0, mask, 0, auto_reset=0, persistent=False))
    for name in _abi.AGENT_KINDS:   # (every workload here has one-port chargers: the RoundRobin_GF agents run on all three)
        a = eng.heuristic_create(name)
        med, ms = timed(lambda: eng.heuristic_run(a, T, None, 0, obs, 0, rew, 0, done, 0, mask, 0))
        print(json.dumps(dict(workload=workload, agent=name, envs=E, ports=P, steps=T, step_kernel=eng.kernel_name,
                              env_steps_per_s=round(E * T / (med / 1e3)), env_steps_per_s_range=[round(E * T / (m / 1e3)) for m in (max(ms), min(ms))],
                              us_per_step=round(med * 1e3 / T, 3), step_only_env_steps_per_s=round(E * T / (step_ms / 1e3)),
                              step_only_us_per_step=round(step_ms * 1e3 / T, 3))), flush=True)
        eng.heuristic_destroy(a)
    eng.close()


def _dispatches(path):
    """(kernel name, start ns, end ns) of every dispatch of a rocprofv3 kernel trace: its CSV output or its SQLite database (rocpd)."""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as c:
            return [(n, int(s), int(e)) for n, s, e in c.execute("select name, start, end from kernels")]
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    col = lambda key: next(c for c in rows[0] if key in c)   # noqa: E731
    kn, k0, k1 = col("Kernel_Name"), col("Start_Timestamp"), col("End_Timestamp")
    return [(r[kn], int(r[k0]), int(r[k1])) for r in rows]


def shares(root):
    """Every agent dispatch is followed by its step dispatch: the agent kernel's share of the pair, per trace and agent."""
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True) +
                   glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel_trace.csv / *_results.db under {root}")
    for f in files:
        acc, pending = {}, None
        for name, t0, t1 in sorted(_dispatches(f), key=lambda d: d[1]):
            dur = (t1 - t0) / 1e3
            m = re.search(r"ev2g_heuristic_kernel<(\d)>", name)
            if m:
                pending = (int(m.group(1)), dur)
            elif pending and "ev2g_step" in name:
                step = re.sub(r"\(.*", "", name).replace("void ", "")
                a = acc.setdefault((AGENTS[pending[0]], step), [0, 0.0, 0.0])
                a[0] += 1
                a[1] += pending[1]
                a[2] += dur
                pending = None
        for (agent, step), (n, h, s) in sorted(acc.items()):
            print(json.dumps(dict(trace=os.path.relpath(f, root), agent=agent, step_kernel=step, pairs=n, agent_us_mean=round(h / n, 3),
                                  step_us_mean=round(s / n, 3), agent_share=round(h / (h + s), 4))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3,cfg4")
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--link", metavar="P_FAIL,P_DELAY", help="time ev2g_link_run under these probabilities next to the plain per-step launches")
    ap.add_argument("--shares", metavar="DIR", help="read rocprofv3 kernel traces under DIR instead of running")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares)
    else:
        for w in args.workloads.split(","):
            if args.link:
                link_rates(w, args.episodes, *[float(x) for x in args.link.split(",")])
            else:
                rates(w, args.episodes)
