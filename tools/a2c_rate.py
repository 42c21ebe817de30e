"""Rate of an A2C loop that stays on the device -- OnPolicyCollector(n_steps=5, gae_lambda=1.0).collect() (rollout, bootstrap value, GAE), then
A2CLearner.train() (ev2g_a2c_update: gradient, reduction, clip + RMSprop + repack, then ev2g_ppo_sync) -- next to the same iterations with the
update done the way a user has today: a torch-on-GPU module pair with autograd, clip_grad_norm_ and torch.optim.RMSprop(alpha=0.99, eps=1e-5)
on the same device batch.  One JSON line per workload.

  python tools/a2c_rate.py [--workloads cfg2,cfg3] [--n-steps 5] [--iterations 200] [--passes 3] [--no-torch]
      wall clock per iteration and of the update alone (medians over --passes passes of --iterations iterations after a warm-up of 20
      iterations), env-steps/s of both loops, and torch_over_device for the update and for the iteration.  The torch loop's collector keeps
      sampling from the device policy's own weights: handing torch's new weights back to the collector is NOT counted, which favours torch.
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/a2c_rate.py --workloads cfg2 --iterations 50 --passes 1 --no-torch
      kernel time of an update: the ev2g_ppo_grad_kernel / ev2g_ppo_reduce_kernel / ev2g_a2c_apply_kernel rows of OUT's kernel statistics

The workloads are bench.py's shapes (tools/heuristic_rate.py WORKLOADS) with SB3's default 64-64 tanh policy.  The figures time the arithmetic,
not learning."""
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


class TorchA2C:
    """SB3's ActorCriticPolicy (two 64-64 tanh trunks, linear heads, log_std) and A2C.train()'s update in torch on the GPU."""

    def __init__(self, weights, log_std, dev, lr=7e-4):
        import torch
        self.torch = torch
        self.p = [torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dev)) for a in list(weights) + [log_std]]
        self.opt = torch.optim.RMSprop(self.p, lr=lr, alpha=0.99, eps=1e-5)

    def update(self, x, a, A, R, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5):
        t, p = self.torch, self.p
        F = t.nn.functional
        mu = F.linear(t.tanh(F.linear(t.tanh(F.linear(x, p[0], p[1])), p[2], p[3])), p[8], p[9])
        v = F.linear(t.tanh(F.linear(t.tanh(F.linear(x, p[4], p[5])), p[6], p[7])), p[10], p[11]).flatten()
        dist = t.distributions.Normal(mu, t.ones_like(mu) * p[12].exp())
        lp, ent = dist.log_prob(a).sum(dim=1), dist.entropy().sum(dim=1)
        loss = -(A * lp).mean() + ent_coef * -ent.mean() + vf_coef * F.mse_loss(R, v)
        self.opt.zero_grad()
        loss.backward()
        t.nn.utils.clip_grad_norm_(self.p, max_grad_norm)
        self.opt.step()


def _passes(n_passes, iterations, warmup, collect, update, sync):
    """[(ms per iteration, ms per update)] of n_passes passes; an iteration = collect() then update(batch), each ended by a synchronisation"""
    out = []
    for k in range(n_passes + 1):
        n = warmup if k == 0 else iterations
        upd = 0.0
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            batch = collect()
            t1 = time.perf_counter()
            update(batch)
            sync()
            upd += time.perf_counter() - t1
        if k:
            out.append(((time.perf_counter() - t0) * 1e3 / n, upd * 1e3 / n))
    return out


def rates(workload, n_steps, iterations, n_passes, with_torch):
    import torch
    from ev2gym_amd.a2c import A2CLearner
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.onpolicy import GaussianActorCritic, OnPolicyCollector, init_ac_weights
    from ev2gym_amd.scenario_gen import generate_native
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    E, P, D = eng.E, eng.P, eng.D
    lo = 0.0 if kinds[1] == "PublicPST" else -1.0
    w0, ls0 = init_ac_weights(D, P, seed=1), np.zeros(P, np.float32)
    pol = GaussianActorCritic(w0, ls0, activation="tanh", lo=lo, seed=2).attach(eng)
    col = OnPolicyCollector(eng, pol, n_steps, gae_lambda=1.0)
    dev = torch.device("cuda", eng.device)
    N = n_steps * E
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731  (collect() and train() end with the engine's own synchronisation)
    learner = A2CLearner(col)
    dpass = _passes(n_passes, iterations, 20, col.collect, learner.train, sync)
    learner.close()
    it, up = statistics.median(p[0] for p in dpass), statistics.median(p[1] for p in dpass)
    line = dict(workload=workload, envs=E, n_steps=n_steps, rows_per_update=N, obs_dim=D, ports=P, iterations=iterations, passes=n_passes,
                device_ms_per_iteration=round(it, 4), device_ms_per_iteration_range=[round(min(p[0] for p in dpass), 4), round(max(p[0] for p in dpass), 4)],
                device_ms_per_update=round(up, 4), device_ms_per_update_range=[round(min(p[1] for p in dpass), 4), round(max(p[1] for p in dpass), 4)],
                device_env_steps_per_s=round(N / (it / 1e3)))
    if with_torch:
        pol.set_weights(w0); pol.set_log_std(ls0)
        ref = TorchA2C(w0, ls0, dev)
        flat = lambda b: ref.update(b.observations.reshape(N, D), b.actions.reshape(N, P), b.advantages.reshape(N), b.returns.reshape(N))  # noqa: E731
        tpass = _passes(n_passes, iterations, 20, col.collect, flat, sync)
        tit, tup = statistics.median(p[0] for p in tpass), statistics.median(p[1] for p in tpass)
        line.update(torch_ms_per_iteration=round(tit, 4), torch_ms_per_update=round(tup, 4),
                    torch_ms_per_update_range=[round(min(p[1] for p in tpass), 4), round(max(p[1] for p in tpass), 4)],
                    torch_env_steps_per_s=round(N / (tit / 1e3)), torch_over_device_update=round(tup / up, 2), torch_over_device_iteration=round(tit / it, 2))
    print(json.dumps(line), flush=True)
    pol.close()
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--n-steps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop")
    args = ap.parse_args()
    for w in args.workloads.split(","):
        rates(w, args.n_steps, args.iterations, args.passes, not args.no_torch)
