"""Rates of the reference's action wrappers applied on the device (ev2g_wrap_run: the wrapper's launch, then a one-step launch of the step
kernel, T times per episode), one JSON line per (workload, wrapper).

  python tools/wrap_rate.py [--workloads cfg2,cfg3] [--episodes 3]
      env-steps/s from HIP-event kernel time (last_step_n_kernel_ms), next to the same one-launch-per-step run with the wrapper's recorded
      output fed as fixed actions (`step_only`): the same trajectory without the wrapper's launches
  rocprofv3 --kernel-trace --stats -d OUT/cfg2 -- python tools/wrap_rate.py --workloads cfg2 --episodes 1
  python tools/wrap_rate.py --shares OUT
      the wrapper kernel's share of each (wrapper + step) pair, from the dispatches of every kernel_trace.csv under OUT

The workloads are bench.py's shapes with one-port chargers; cfg2 is drawn with power setpoints (its config has none, and the repair layer
works towards the step's setpoint).  Raw actions: uniform(0, 1) from the engine's counter-based generator (ThreeStep_Action: the levels 0 / 1 / 2).
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from ev2gym_amd import _abi  # noqa: E402
from heuristic_rate import WORKLOADS, _dispatches  # noqa: E402

KINDS = ("BinaryAction", "ThreeStep_Action", "Rescale_RepairLayer")


def rates(workload, episodes):
    from ev2gym_amd.engine import Engine, host_uniform
    from ev2gym_amd.scenario_gen import generate_native
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    obs, rew = eng.empty((E, D)), eng.empty((E,))
    done, mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    raw, wrapped = eng.empty((T, E, P)), eng.empty((T, E, P))
    out = (obs, 0, rew, 0, done, 0, mask, 0)

    def timed(run):
        ms = []
        for i in range(episodes + 1):   # the first episode warms up
            eng.reset()
            run()
            if i:
                ms.append(eng.last_step_n_kernel_ms())
        eng.check_faults()
        return statistics.median(ms), ms

    rate = lambda m: round(E * T / (m / 1e3))   # noqa: E731
    for name in KINDS:
        u = host_uniform(T * E * P, 77, 0.0, 1.0)
        raw.upload((np.floor(u * 3.0) if name == "ThreeStep_Action" else u).reshape(T, E, P))
        w = eng.wrap_create(name)

        def wrapped_run():
            eng.wrap_reset_state(w)
            eng.wrap_run(w, T, raw, E * P, wrapped, E * P, *out)

        med, ms = timed(wrapped_run)
        # the recorded wrapped actions drive the same trajectory through plain one-step launches
        step_ms, _ = timed(lambda: eng.step_n(T, wrapped, E * P, *out, auto_reset=0, persistent=False))
        print(json.dumps(dict(workload=workload, wrapper=name, envs=E, ports=P, steps=T, step_kernel=eng.kernel_name,
                              env_steps_per_s=rate(med), env_steps_per_s_range=[rate(max(ms)), rate(min(ms))],
                              us_per_step=round(med * 1e3 / T, 3), step_only_env_steps_per_s=rate(step_ms),
                              step_only_us_per_step=round(step_ms * 1e3 / T, 3), wrapped_over_step_only=round(med / step_ms, 4))), flush=True)
        eng.wrap_destroy(w)
    eng.close()


def shares(root):
    """Every wrapper dispatch is followed by its step dispatch: the wrapper kernel's share of the pair, per trace and wrapper kernel."""
    import glob
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True) +
                   glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel_trace.csv / *_results.db under {root}")
    for f in files:
        acc, pending = {}, None
        for name, t0, t1 in sorted(_dispatches(f), key=lambda d: d[1]):
            dur = (t1 - t0) / 1e3
            m = re.search(r"(ev2g_wrap_\w+_kernel<\w+>)", name)
            if m:
                pending = (m.group(1), dur)
            elif pending and "ev2g_step" in name:
                step = re.sub(r"\(.*", "", name).replace("void ", "")
                a = acc.setdefault((pending[0], step), [0, 0.0, 0.0])
                a[0] += 1
                a[1] += pending[1]
                a[2] += dur
                pending = None
        for (kern, step), (n, h, s) in sorted(acc.items()):
            print(json.dumps(dict(trace=os.path.relpath(f, root), wrapper_kernel=kern, step_kernel=step, pairs=n, wrapper_us_mean=round(h / n, 3),
                                  step_us_mean=round(s / n, 3), wrapper_share=round(h / (h + s), 4))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--shares", metavar="DIR", help="read rocprofv3 kernel traces under DIR instead of running")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares)
    else:
        for w in args.workloads.split(","):
            rates(w, args.episodes)
