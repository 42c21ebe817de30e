"""Wall clock and kernel time of ARS on the device (ev2gym_amd/ars.py, csrc/ev2g_ars.h), one JSON line per (workload, n_delta):

  * a whole-episode rollout under the POPULATION actor (2 n_delta weight images, one launch per step) next to the same loop under ONE shared
    image -- ev2g_ars_rollout in centre mode, and ev2g_ac_collect deterministic: the difference prices the per-candidate weight stream;
    wall clock per step, and HIP-event time of the whole call per step (Engine.last_step_n_kernel_ms);
  * a whole iteration, perturb + episode + update (ARSLearner.train()), next to torch-on-GPU doing the same arithmetic over the same engine:
    a torch.bmm population forward per step, the float32 hand-over step, and sb3_contrib's update lines.

  python tools/ars_rate.py [--workloads cfg2,cfg3] [--n-delta 8,64,half] [--passes 3] [--no-torch]      medians of --passes episodes after a warm-up
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/ars_rate.py --workloads cfg2 --n-delta 64 --passes 1 --no-torch
      kernel time per launch: the ev2g_ars_* rows of OUT's kernel statistics (counters, --pmc, in a run of their own)

The workloads are bench.py's shapes (tools/heuristic_rate.py WORKLOADS) with sb3_contrib's default 64-64 MlpPolicy.  The figures time the
arithmetic, not learning."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from ev2gym_amd import _abi  # noqa: E402
from heuristic_rate import WORKLOADS  # noqa: E402


def _median(n_passes, run, sync):
    """(median wall ms, [min, max], median of what run() returns) over n_passes runs after one warm-up"""
    wall, extra = [], []
    for k in range(n_passes + 1):
        sync()
        t0 = time.perf_counter()
        x = run()
        sync()
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
            extra.append(x)
    return round(statistics.median(wall), 4), [round(min(wall), 4), round(max(wall), 4)], (round(statistics.median(extra), 4) if extra[0] is not None else None)


def rates(workload, n_delta, n_passes, with_torch):
    import torch
    from ev2gym_amd.ars import ARSLearner
    from ev2gym_amd.engine import Engine, ars_query
    from ev2gym_amd.onpolicy import GaussianActorCritic, init_ac_weights
    from ev2gym_amd.scenario_gen import generate_native
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    lo = 0.0 if kinds[1] == "PublicPST" else -1.0
    nd = E // 2 if n_delta == "half" else int(n_delta)
    learner = ARSLearner(eng, n_delta=nd, seed=3, lo=lo)
    ars, obs32 = learner.ars, learner.obs32
    dev = torch.device("cuda", eng.device)
    sync = lambda: (eng.synchronize(), torch.cuda.synchronize(dev))   # noqa: E731
    info = ars_query("MlpPolicy", D, 64, 64, P, None)
    eng.ars_perturb(ars)

    def episode(population):
        eng.reset_f32(obs32, 0)
        eng.ars_rollout(ars, T, population=population)
        eng.synchronize()
        return eng.last_step_n_kernel_ms()

    pop_ms, pop_rng, pop_ev = _median(n_passes, lambda: episode(True), sync)
    one_ms, one_rng, one_ev = _median(n_passes, lambda: episode(False), sync)
    # the same loop under the Gaussian actor-critic's deterministic collector (one shared image, both trunks)
    pol = GaussianActorCritic(init_ac_weights(D, P, seed=1), np.zeros(P, np.float32), activation="tanh", lo=lo, seed=2).attach(eng)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    rows = (z((T + 1, E, D), torch.float32), z((T, E, P), torch.float32), z((T, E), torch.float32), z((T, E), torch.float32), z((T, E), torch.float64),
            z((T, E), torch.uint8), z((T, E, P), torch.uint8))

    def ac_episode():
        eng.reset_f32(rows[0][0], 0)
        eng.ac_collect(pol.ac, T, *rows, deterministic=True)
        eng.synchronize()
        return eng.last_step_n_kernel_ms()

    ac_ms, ac_rng, ac_ev = _median(n_passes, ac_episode, sync)
    it_ms, it_rng, _ = _median(n_passes, lambda: (learner.train(first_offset=0), None)[1], sync)
    line = dict(workload=workload, envs=E, steps=T, obs_dim=D, ports=P, n_delta=nd, candidates=2 * nd, rows_per_candidate=E // (2 * nd), passes=n_passes,
                candidate_image_bytes=4 * info["candidate_floats"], lds_bytes=info["lds_bytes"],
                population_wall_us_per_step=round(pop_ms * 1e3 / T, 3), population_wall_ms_range=pop_rng, population_event_us_per_step=round(pop_ev * 1e3 / T, 3),
                centre_wall_us_per_step=round(one_ms * 1e3 / T, 3), centre_wall_ms_range=one_rng, centre_event_us_per_step=round(one_ev * 1e3 / T, 3),
                ac_collect_wall_us_per_step=round(ac_ms * 1e3 / T, 3), ac_collect_wall_ms_range=ac_rng, ac_collect_event_us_per_step=round(ac_ev * 1e3 / T, 3),
                iteration_wall_ms=it_ms, iteration_wall_ms_range=it_rng, launches_per_iteration=1 + 2 * T + 1 + 3)
    pol.close()
    if with_torch:
        n = info["n_params"]
        R = E // (2 * nd)
        shapes = _abi.ars_param_shapes("MlpPolicy", D, 64, 64, P)
        theta = torch.zeros(n, device=dev)
        x_obs, x_act = z((E, D), torch.float32), z((E, P), torch.float32)
        rew, done, mask = z((T, E), torch.float64), z((E,), torch.uint8), z((E, P), torch.uint8)

        def torch_iteration():
            delta = torch.randn(nd, n, device=dev)
            cand = torch.cat([theta + 0.05 * delta, theta - 0.05 * delta])
            w, o = [], 0
            for s in shapes:
                k = int(np.prod(s))
                w.append(cand[:, o:o + k].reshape(2 * nd, *s))
                o += k
            eng.set_extras(obs_f32=x_obs, actions_f32=x_act)
            eng.reset_f32(x_obs, 0)
            for t in range(T):
                eng.synchronize()   # the engine's stream and torch's are two streams
                x = x_obs.view(2 * nd, R, D)
                h = torch.relu(torch.baddbmm(w[1][:, None, :], x, w[0].transpose(1, 2)))
                h = torch.relu(torch.baddbmm(w[3][:, None, :], h, w[2].transpose(1, 2)))
                a = torch.tanh(torch.baddbmm(w[5][:, None, :], h, w[4].transpose(1, 2)))
                x_act.copy_((0.5 * (a + 1.0) if lo == 0.0 else a).reshape(E, P))
                torch.cuda.synchronize(dev)
                eng.step_n(1, None, 0, None, 0, rew[t], 0, done, 0, mask, 0, auto_reset=False, persistent=False)
            eng.synchronize()
            eng.set_extras()
            r = rew.sum(0).view(2 * nd, R).sum(1)
            plus, minus = r[:nd], r[nd:]
            top, _ = torch.max(torch.vstack((plus, minus)), dim=0)
            idx = torch.argsort(top, descending=True)[:nd]
            std = torch.cat([plus[idx], minus[idx]]).std()
            theta.add_((0.02 / (nd * std + 1e-6)) * ((plus[idx] - minus[idx]).float() @ delta[idx]))

        t_ms, t_rng, _ = _median(n_passes, torch_iteration, sync)
        line.update(torch_iteration_wall_ms=t_ms, torch_iteration_wall_ms_range=t_rng, torch_over_device_iteration=round(t_ms / it_ms, 2))
    print(json.dumps(line), flush=True)
    learner.close()
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--n-delta", default="8,64,half")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop")
    args = ap.parse_args()
    for w in args.workloads.split(","):
        for nd in args.n_delta.split(","):
            rates(w, nd, args.passes, not args.no_torch)
