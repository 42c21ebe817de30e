"""Rate of ev2g_rollout over unfused, graph-captured segments: the cfg2 shape (4096 envs x 50 chargers, one transformer) under a seeded
D -> 64 -> 64 -> P bf16 actor (not the fused launch's packing, so every step is an actor launch and a step launch), episodes of T / k
segments of k steps, one JSON line.

  python tools/rollout_rate.py [--k 8] [--episodes 7]
      env-steps/s from HIP-event time (the sum of the segments' step_n_kernel_ms_back readings) and from wall clock between device
      synchronisations, median of the episodes after the first two; rollout_graph_launches after episodes 1 and 2 (the first episode
      captures every segment and launches it, the second only launches: k >= 4 is what ev2g_rollout captures)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ev2gym_amd import _abi  # noqa: E402
from ev2gym_amd.scenario_gen import GenConfig  # noqa: E402


def rates(k, episodes):
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.scenario_gen import generate_native
    eng = Engine(generate_native(GenConfig.v2g_profit_plus_loads(4096, 50, 1, seed=1234)), _abi.REWARD_KINDS["ProfitMax_TrPenalty_UserIncentives"],
                 _abi.STATE_KINDS["V2G_profit_max_loads"], flags=_abi.FLAG_LOG_SOC)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    o32, a32 = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
    eng.set_extras(obs_f32=o32, actions_f32=a32)
    mlp = eng.mlp_create(*init_mlp_weights(D, P, seed=9, h1=64, h2=64), out_lo=-1.0)
    rew, done, mask = eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    segs = T // k
    assert 1 <= segs <= 32   # (the handle keeps the readings of its last 32 timed calls)
    ev_ms, wall_ms, launches = [], [], []
    for _ in range(episodes):
        eng.reset()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(segs):
            eng.rollout(mlp, k, rew, 0, done, 0, mask, 0)
        eng.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms.append(sum(eng.step_n_kernel_ms_back(b) for b in range(segs)))
        launches.append(eng.rollout_graph_launches)
    eng.check_faults()
    assert eng.last_launch_specialisation != 4   # (4: the fused launch)
    rate = lambda ms: round(E * segs * k / (ms / 1e3))   # noqa: E731
    print(json.dumps(dict(measure="rollout_graphs", envs=E, ports=P, k=k, segments=segs, step_kernel=eng.kernel_name,
                          graph_launches_after_episode=launches[:2], ev_env_steps_per_s=rate(float(np.median(ev_ms[2:]))),
                          ev_range=[rate(max(ev_ms[2:])), rate(min(ev_ms[2:]))], wall_env_steps_per_s=rate(float(np.median(wall_ms[2:]))))), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--episodes", type=int, default=7)
    args = ap.parse_args()
    rates(args.k, max(args.episodes, 3))
