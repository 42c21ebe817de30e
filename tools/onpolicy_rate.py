"""Rate of on-policy rollout collection on the device (ev2g_ac_collect: the Gaussian actor-critic's sampling launch, then a one-step launch of the
step kernel, T times per episode) with SB3's default 64-64 tanh policy, one JSON line per workload.

  python tools/onpolicy_rate.py [--workloads cfg2,cfg3] [--episodes 3]
      env-steps/s of ev2g_ac_collect from HIP-event kernel time (last_step_n_kernel_ms) and from wall-clock time, next to the same per-step
      loop with a torch nn.Sequential pair doing forward, sample and log-prob between the float32 hand-over buffers (wall clock: a dozen
      launches per step from Python, and TWO host synchronisations per step -- torch's stream before the engine's step, the engine's after
      it -- that the collect call never pays: `collect_over_torch_wall` compares the two loops as a user would run them, not two kernels)
  rocprofv3 --kernel-trace --stats -d OUT/cfg2 -- python tools/onpolicy_rate.py --workloads cfg2 --episodes 1 --no-torch
  python tools/onpolicy_rate.py --shares OUT
      the act kernel's share of a step's kernel time, from the dispatches of every kernel trace under OUT (one clock: the trace's)

The workloads are bench.py's shapes (tools/heuristic_rate.py WORKLOADS).  Random weights, log_std 0, no learner.
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from ev2gym_amd import _abi  # noqa: E402
from heuristic_rate import WORKLOADS, _dispatches  # noqa: E402


def torch_pair(weights, dev):
    import torch
    nn = torch.nn
    w = [torch.from_numpy(a).to(dev) for a in weights]

    def seq(i0, head):
        lins = []
        for W, b in ((w[i0], w[i0 + 1]), (w[i0 + 2], w[i0 + 3]), (w[head], w[head + 1])):
            lin = nn.Linear(W.shape[1], W.shape[0]).to(dev)
            with torch.no_grad():
                lin.weight.copy_(W); lin.bias.copy_(b)
            lins.append(lin)
        return nn.Sequential(lins[0], nn.Tanh(), lins[1], nn.Tanh(), lins[2])
    return seq(0, 8), seq(4, 10)


def rates(workload, episodes, with_torch):
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.onpolicy import GaussianActorCritic, init_ac_weights
    from ev2gym_amd.scenario_gen import generate_native
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    lo = 0.0 if kinds[1] == "PublicPST" else -1.0
    pol = GaussianActorCritic(init_ac_weights(D, P, seed=1), np.zeros(P, np.float32), activation="tanh", lo=lo, seed=2).attach(eng)
    obs, act = eng.empty((T + 1, E, D), np.float32), eng.empty((T, E, P), np.float32)
    val, lp = eng.empty((T, E), np.float32), eng.empty((T, E), np.float32)
    rew, done, mask = eng.empty((T, E)), eng.empty((T, E), np.uint8), eng.empty((T, E, P), np.uint8)
    ms, wall = [], []
    for i in range(episodes + 1):   # the first episode warms up
        eng.reset_f32(obs, 0)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.ac_collect(pol.ac, T, obs, act, val, lp, rew, done, mask)
        eng.synchronize()
        if i:
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.last_step_n_kernel_ms())
    eng.check_faults()
    spec = eng.last_launch_specialisation
    med, wmed = statistics.median(ms), statistics.median(wall)
    rate = lambda m: round(E * T / (m / 1e3))   # noqa: E731
    line = dict(workload=workload, envs=E, ports=P, obs_dim=D, steps=T, policy=f"{D}->64->64->{P} + {D}->64->64->1 tanh", step_kernel=eng.kernel_name,
                last_launch_specialisation=spec, env_steps_per_s=rate(med), env_steps_per_s_range=[rate(max(ms)), rate(min(ms))],
                us_per_step=round(med * 1e3 / T, 3), wall_env_steps_per_s=rate(wmed))
    if with_torch:
        import torch
        dev = torch.device("cuda", eng.device)
        pi, vf = torch_pair(pol.weights, dev)
        log_std = torch.zeros(P, device=dev)
        o32, a32 = torch.zeros((E, D), dtype=torch.float32, device=dev), torch.zeros((E, P), dtype=torch.float32, device=dev)
        t_rew, t_done, t_mask = eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
        eng.set_extras(obs_f32=o32, actions_f32=a32)
        twall = []
        for i in range(episodes + 1):
            eng.reset_f32(o32, 0)
            eng.synchronize()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.no_grad():
                for _ in range(T):
                    dist = torch.distributions.Normal(pi(o32), log_std.exp())
                    a = dist.sample()
                    logp = dist.log_prob(a).sum(dim=1)   # noqa: F841  (what the buffer would store)
                    v = vf(o32)                          # noqa: F841
                    a32.copy_(a.clamp(lo, 1.0))
                    torch.cuda.synchronize(dev)          # the engine steps on its own stream
                    eng.step_n(1, None, 0, None, 0, t_rew, 0, t_done, 0, t_mask, 0, auto_reset=False, persistent=False)
                    eng.synchronize()
            if i:
                twall.append((time.perf_counter() - t0) * 1e3)
        eng.set_extras()
        tmed = statistics.median(twall)
        line.update(torch_wall_env_steps_per_s=rate(tmed), collect_over_torch_wall=round(tmed / wmed, 2))
    print(json.dumps(line), flush=True)
    pol.close()
    eng.close()


def shares(root):
    """Every sampling dispatch is followed by its step dispatch: the act kernel's share of the pair, per trace."""
    import glob
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True) +
                   glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel_trace.csv / *_results.db under {root}")
    for f in files:
        acc, pending = {}, None
        for name, t0, t1 in sorted(_dispatches(f), key=lambda d: d[1]):
            dur = (t1 - t0) / 1e3
            m = re.search(r"(ev2g_ac_act_kernel<\w+>)", name)
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
            print(json.dumps(dict(trace=os.path.relpath(f, root), act_kernel=kern, step_kernel=step, pairs=n, act_us_mean=round(h / n, 3),
                                  step_us_mean=round(s / n, 3), act_share=round(h / (h + s), 4))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison loop")
    ap.add_argument("--shares", metavar="DIR", help="read rocprofv3 kernel traces under DIR instead of running")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares)
    else:
        for w in args.workloads.split(","):
            rates(w, args.episodes, not args.no_torch)
