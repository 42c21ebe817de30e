"""Wall clock of a TRPO update that stays on the device -- TRPOLearner.train() on one collected rollout: ev2g_trpo_policy_step (gradient, up to
15 Fisher-vector products with their conjugate-gradient iterations, the line search; about 100 launches, no host round trip), then
n_critic_updates passes of ev2g_trpo_critic_minibatch, then ev2g_ppo_sync -- next to the same update done the way a user has today: torch-on-GPU
modules doing exactly what sb3_contrib's TRPO.train() does (KL from torch.distributions, H v by double backward, a Python conjugate gradient and
line search with their .item() synchronisations, torch.optim.Adam on the value function).  One JSON line per (workload, sub_sampling_factor).

  python tools/trpo_rate.py [--workloads cfg2,cfg3] [--n-steps 96] [--sub-sampling 1,8] [--repeats 5] [--passes 3] [--no-torch]
      the policy step alone and the whole train(), medians over --passes passes of --repeats updates of the SAME rollout from the SAME starting
      weights (set back before every update, outside the clock), after one warm-up update; torch_over_device for both.
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/trpo_rate.py --workloads cfg2 --repeats 2 --passes 1 --no-torch
      kernel time per launch: the ev2g_trpo_* rows of OUT's kernel statistics

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

ACTOR = _abi.TRPO_ACTOR
VALUE = (4, 5, 6, 7, 10, 11)


class TorchTRPO:
    """sb3_contrib's TRPO.train() for ActorCriticPolicy (two 64-64 tanh trunks, linear heads, log_std) in torch on the GPU."""

    def __init__(self, weights, log_std, dev, lr=1e-3):
        import torch
        self.torch = torch
        self.p = [torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dev)) for a in list(weights) + [log_std]]
        self.actor, self.vals = [self.p[i] for i in ACTOR], [self.p[i] for i in VALUE]
        self.opt = torch.optim.Adam(self.vals, lr=lr, eps=1e-5)

    def reset(self, weights, log_std):
        with self.torch.no_grad():
            for p, a in zip(self.p, list(weights) + [log_std]):
                p.copy_(self.torch.from_numpy(np.array(a)))
        self.opt = self.torch.optim.Adam(self.vals, lr=self.opt.param_groups[0]["lr"], eps=1e-5)

    def dist(self, x):
        t, p = self.torch, self.p
        F = t.nn.functional
        mu = F.linear(t.tanh(F.linear(t.tanh(F.linear(x, p[0], p[1])), p[2], p[3])), p[8], p[9])
        return t.distributions.Normal(mu, t.ones_like(mu) * p[12].exp())

    def policy_step(self, x, a, old_lp, adv, target_kl=0.01, damping=0.1, cg_max_steps=15, shrink=0.8, ls_max_iter=10):
        t = self.torch
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        d = self.dist(x)
        old = t.distributions.Normal(d.loc.detach(), d.scale.detach())
        J0 = (adv * t.exp(d.log_prob(a).sum(dim=1) - old_lp)).mean()
        g = t.cat([v.reshape(-1) for v in t.autograd.grad(J0, self.actor, retain_graph=True)])
        gkl = t.cat([v.reshape(-1) for v in t.autograd.grad(t.distributions.kl_divergence(d, old).sum(dim=1).mean(), self.actor, create_graph=True)])

        def hvp(v):
            return t.cat([h.reshape(-1) for h in t.autograd.grad((gkl * v).sum(), self.actor, retain_graph=True)]) + damping * v

        xs, r, p = t.zeros_like(g), g.clone(), g.clone()
        rho = r @ r
        if rho.item() >= 1e-10:
            for i in range(cg_max_steps):
                Hp = hvp(p)
                alpha = rho / (p @ Hp)
                xs += alpha * p
                if i == cg_max_steps - 1:
                    break
                r -= alpha * Hp
                new = r @ r
                if new.item() < 1e-10:
                    break
                p = r + (new / rho) * p
                rho = new
        beta = t.sqrt(2 * target_kl / (xs @ hvp(xs)))
        theta0 = [q.detach().clone() for q in self.actor]
        c, ok = 1.0, False
        with t.no_grad():
            for _ in range(ls_max_iter):
                o = 0
                for q, q0 in zip(self.actor, theta0):
                    q.copy_(q0 + c * beta * xs[o:o + q.numel()].reshape(q.shape))
                    o += q.numel()
                d = self.dist(x)
                J = (adv * t.exp(d.log_prob(a).sum(dim=1) - old_lp)).mean()
                kl = t.distributions.kl_divergence(d, old).sum(dim=1).mean()
                if kl.item() < target_kl and J.item() > J0.item():
                    ok = True
                    break
                c *= shrink
            if not ok:
                for q, q0 in zip(self.actor, theta0):
                    q.copy_(q0)
        return ok

    def critic(self, x, R, pieces):
        t, p = self.torch, self.p
        F = t.nn.functional
        for ix in pieces:
            xi = x[ix]
            v = F.linear(t.tanh(F.linear(t.tanh(F.linear(xi, p[4], p[5])), p[6], p[7])), p[10], p[11]).flatten()
            loss = F.mse_loss(R[ix], v)
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()


def _median_ms(n_passes, repeats, reset, run, sync):
    out = []
    for k in range(n_passes + 1):
        n, total = (1 if k == 0 else repeats), 0.0
        for _ in range(n):
            reset()
            sync()
            t0 = time.perf_counter()
            run()
            sync()
            total += time.perf_counter() - t0
        if k:
            out.append(total * 1e3 / n)
    return round(statistics.median(out), 4), [round(min(out), 4), round(max(out), 4)]


def rates(workload, n_steps, factor, repeats, n_passes, with_torch):
    import torch
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.onpolicy import GaussianActorCritic, OnPolicyCollector, init_ac_weights
    from ev2gym_amd.scenario_gen import generate_native
    from ev2gym_amd.trpo import TRPOLearner
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    E, P, D = eng.E, eng.P, eng.D
    lo = 0.0 if kinds[1] == "PublicPST" else -1.0
    w0, ls0 = init_ac_weights(D, P, seed=1), np.zeros(P, np.float32)
    pol = GaussianActorCritic(w0, ls0, activation="tanh", lo=lo, seed=2).attach(eng)
    col = OnPolicyCollector(eng, pol, n_steps)
    dev = torch.device("cuda", eng.device)
    N = n_steps * E
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    batch = col.collect().clone()
    learner = TRPOLearner(col, sub_sampling_factor=factor, seed=3)
    gen_t = torch.Generator(device=dev)
    gen_t.manual_seed(3)
    rows = (torch.randperm(N, generator=gen_t, device=dev)[::factor] if factor > 1 else torch.arange(N, device=dev)).to(torch.int32).contiguous()
    perms = [torch.randperm(N, generator=gen_t, device=dev).to(torch.int32) for _ in range(10)]
    pieces = [p[i:i + 128] for p in perms for i in range(0, N, 128)]
    obs, act, old, adv, ret = learner._flat(batch, N, "log_probs", "advantages", "returns")

    def reset():
        pol.set_weights(w0); pol.set_log_std(ls0)

    def step():
        eng.trpo_policy_step(learner.trpo, obs, act, old, adv, rows, rows.numel())
        learner.last = eng.trpo_get_report(learner.trpo)

    step_ms, step_rng = _median_ms(n_passes, repeats, reset, step, sync)
    train_ms, train_rng = _median_ms(n_passes, repeats, reset, lambda: learner.train(batch, policy_rows=rows, minibatches=pieces), sync)
    line = dict(workload=workload, envs=E, n_steps=n_steps, rows=N, sub_sampling_factor=factor, policy_rows=int(rows.numel()), critic_minibatches=len(pieces),
                obs_dim=D, ports=P, repeats=repeats, passes=n_passes, device_ms_policy_step=step_ms, device_ms_policy_step_range=step_rng,
                device_ms_train=train_ms, device_ms_train_range=train_rng, device_report=learner.last)
    learner.close()
    if with_torch:
        ref = TorchTRPO(w0, ls0, dev)
        r64, p64 = rows.long(), [ix.long() for ix in pieces]
        xr, ar, oldr, advr = obs[r64], act[r64], old[r64], adv[r64]
        rs = lambda: ref.reset(w0, ls0)   # noqa: E731
        t_step, t_step_rng = _median_ms(n_passes, repeats, rs, lambda: ref.policy_step(xr, ar, oldr, advr), sync)
        t_train, t_train_rng = _median_ms(n_passes, repeats, rs, lambda: (ref.policy_step(xr, ar, oldr, advr), ref.critic(obs, ret, p64)), sync)
        line.update(torch_ms_policy_step=t_step, torch_ms_policy_step_range=t_step_rng, torch_ms_train=t_train, torch_ms_train_range=t_train_rng,
                    torch_over_device_policy_step=round(t_step / step_ms, 2), torch_over_device_train=round(t_train / train_ms, 2))
    print(json.dumps(line), flush=True)
    pol.close()
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--n-steps", type=int, default=96)
    ap.add_argument("--sub-sampling", default="1,8")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop")
    args = ap.parse_args()
    for w in args.workloads.split(","):
        for f in args.sub_sampling.split(","):
            rates(w, args.n_steps, int(f), args.repeats, args.passes, not args.no_torch)
