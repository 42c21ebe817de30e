"""Time of PPOLearner.train() on one collected rollout (ev2g_ppo_minibatch: advantage statistics, gradient, reduction, clip + Adam + repack -- four
launches per minibatch, no host round trip) next to the loop a user has today: the SAME minibatches through a torch-on-GPU nn.Module pair with
autograd, clip_grad_norm_ and torch.optim.Adam(eps=1e-5).  One JSON line per (workload, batch_size).

  python tools/ppo_train_rate.py [--workloads cfg2,cfg3] [--n-steps 96] [--batch-sizes 64,4096,32768] [--reps 5] [--max-minibatches 256] [--no-torch]
      wall clock per minibatch (medians over --reps passes after one warm-up pass; a pass = the first --max-minibatches pieces of one
      permutation of the rollout's rows, the same pieces on both sides), rows/s, and torch_over_device
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/ppo_train_rate.py --workloads cfg2 --batch-sizes 4096 --reps 2 --no-torch
      kernel time: the ev2g_ppo_* rows of OUT's kernel statistics (one clock: the trace's)

The workloads are bench.py's shapes (tools/heuristic_rate.py WORKLOADS) with SB3's default 64-64 tanh policy.  Both sides start every batch size
from the same weights; the figures time the arithmetic, not learning."""
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


class TorchPPO:
    """SB3's ActorCriticPolicy (two 64-64 tanh trunks, linear heads, log_std) and PPO.train()'s minibatch step in torch on the GPU."""

    def __init__(self, weights, log_std, dev, lr=3e-4):
        import torch
        self.torch = torch
        self.p = [torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dev)) for a in list(weights) + [log_std]]
        self.opt = torch.optim.Adam(self.p, lr=lr, eps=1e-5)

    def minibatch(self, obs, actions, old_lp, adv, ret, idx, clip=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5):
        t, p = self.torch, self.p
        F = t.nn.functional
        x, a, old, A, R = obs[idx], actions[idx], old_lp[idx], adv[idx], ret[idx]
        mu = F.linear(t.tanh(F.linear(t.tanh(F.linear(x, p[0], p[1])), p[2], p[3])), p[8], p[9])
        v = F.linear(t.tanh(F.linear(t.tanh(F.linear(x, p[4], p[5])), p[6], p[7])), p[10], p[11]).flatten()
        dist = t.distributions.Normal(mu, t.ones_like(mu) * p[12].exp())
        lp, ent = dist.log_prob(a).sum(dim=1), dist.entropy().sum(dim=1)
        if len(A) > 1:
            A = (A - A.mean()) / (A.std() + 1e-8)
        r = t.exp(lp - old)
        loss = -t.min(A * r, A * t.clamp(r, 1 - clip, 1 + clip)).mean() + ent_coef * -ent.mean() + vf_coef * F.mse_loss(R, v)
        self.opt.zero_grad()
        loss.backward()
        t.nn.utils.clip_grad_norm_(self.p, max_grad_norm)
        self.opt.step()


def rates(workload, n_steps, batch_sizes, reps, max_mb, with_torch):
    import torch
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.onpolicy import GaussianActorCritic, OnPolicyCollector, init_ac_weights
    from ev2gym_amd.ppo import PPOLearner
    from ev2gym_amd.scenario_gen import generate_native
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    E, P, D = eng.E, eng.P, eng.D
    lo = 0.0 if kinds[1] == "PublicPST" else -1.0
    w0, ls0 = init_ac_weights(D, P, seed=1), np.zeros(P, np.float32)
    pol = GaussianActorCritic(w0, ls0, activation="tanh", lo=lo, seed=2).attach(eng)
    col = OnPolicyCollector(eng, pol, min(n_steps, eng.T))
    batch = col.collect().clone()
    N = col.n_steps * E
    dev = batch.observations.device
    flat = [batch.observations.reshape(N, D), batch.actions.reshape(N, P), batch.log_probs.reshape(N), batch.advantages.reshape(N), batch.returns.reshape(N)]
    for bs in batch_sizes:
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(bs)).to(dev)
        pieces = [perm[i:i + bs] for i in range(0, N, bs)][:max_mb]
        rows = sum(len(p) for p in pieces)
        learner = PPOLearner(col, n_epochs=1, batch_size=bs)
        pieces32 = [p.to(torch.int32) for p in pieces]
        wall = []
        for i in range(reps + 1):   # the first pass warms up
            pol.set_weights(w0); pol.set_log_std(ls0)   # (the masters follow; Adam's moments carry over, which costs the same)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            learner.train(batch, minibatches=pieces32)   # (ends with ev2g_ppo_sync, which synchronises)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        learner.close()
        med = statistics.median(wall)
        line = dict(workload=workload, envs=E, n_steps=col.n_steps, rollout_rows=N, obs_dim=D, ports=P, batch_size=bs, minibatches=len(pieces), reps=reps,
                    device_ms_per_minibatch=round(med / len(pieces), 4), device_ms_range=[round(min(wall) / len(pieces), 4), round(max(wall) / len(pieces), 4)],
                    device_rows_per_s=round(rows / (med / 1e3)))
        if with_torch:
            twall = []
            for i in range(reps + 1):
                ref = TorchPPO(w0, ls0, dev)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for ix in pieces:
                    ref.minibatch(*flat, ix)
                torch.cuda.synchronize(dev)
                if i:
                    twall.append((time.perf_counter() - t0) * 1e3)
            tmed = statistics.median(twall)
            line.update(torch_ms_per_minibatch=round(tmed / len(pieces), 4), torch_rows_per_s=round(rows / (tmed / 1e3)), torch_over_device=round(tmed / med, 2))
        print(json.dumps(line), flush=True)
    pol.close()
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--n-steps", type=int, default=96)
    ap.add_argument("--batch-sizes", default="64,4096,32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-minibatches", type=int, default=256)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop")
    args = ap.parse_args()
    for w in args.workloads.split(","):
        rates(w, args.n_steps, [int(b) for b in args.batch_sizes.split(",")], args.reps, args.max_minibatches, not args.no_torch)
