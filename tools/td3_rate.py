"""Wall clock of one TD3 / DDPG update on the device (ev2g_td3_update, with and without the device sampler ev2g_replay_sample in front of it)
next to the same batch through a torch-on-GPU module set with autograd and torch.optim.Adam(eps=1e-8).  One JSON line per (workload, algorithm,
batch size).

  python tools/td3_rate.py [--workloads cfg2,cfg3] [--batches 100,256,1024] [--updates 200] [--passes 3] [--no-torch]
      microseconds per update: medians over --passes passes of --updates updates after a warm-up of 20, each pass ended by ONE synchronisation (the
      updates of a pass are queued back to back, as TD3Learner.train() queues them).  The replay ring is one collected episode of the workload.
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/td3_rate.py --workloads cfg2 --batches 256 --updates 50 --passes 1 --no-torch
      kernel time of an update: the ev2g_td3_* and ev2g_replay_sample_kernel rows of OUT's kernel statistics

The workloads are bench.py's shapes (tools/heuristic_rate.py WORKLOADS) with the reference script's 400-300 networks.  There is no rate threshold:
the figures time the arithmetic, not learning."""
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


class TorchTD3:
    """SB3's TD3Policy (400-300 ReLU actor with tanh, n critics) and TD3.train()'s gradient step in torch on the GPU."""

    def __init__(self, actor, critics, dev, lo, delay, sigma, lr=1e-3, tau=0.005, gamma=0.99, clip=0.5):
        import torch
        self.torch, self.lo, self.delay, self.sigma, self.tau, self.gamma, self.clip, self.n = torch, lo, delay, sigma, tau, gamma, clip, 0
        mk = lambda ws, grad: [torch.from_numpy(np.array(a)).to(dev).requires_grad_(grad) for a in ws]  # noqa: E731
        self.actor, self.critics = mk(actor, True), [mk(c, True) for c in critics]
        self.actor_t, self.critics_t = mk(actor, False), [mk(c, False) for c in critics]
        self.opt_a = torch.optim.Adam(self.actor, lr=lr, eps=1e-8)
        self.opt_c = torch.optim.Adam([a for c in self.critics for a in c], lr=lr, eps=1e-8)

    def _mlp(self, w, x, tanh):
        t = self.torch
        F = t.nn.functional
        z = F.linear(t.relu(F.linear(t.relu(F.linear(x, w[0], w[1])), w[2], w[3])), w[4], w[5])
        return t.tanh(z) if tanh else z

    def update(self, s, a, r, s2, d):
        t = self.torch
        F = t.nn.functional
        self.n += 1
        if self.lo == 0.0:
            a = 2.0 * a - 1.0
        with t.no_grad():
            at = self._mlp(self.actor_t, s2, True)
            if self.sigma > 0.0:
                at = at + (t.randn_like(at) * self.sigma).clamp(-self.clip, self.clip)
            xa2 = t.cat([s2, at.clamp(-1.0, 1.0)], 1)
            y = r + (1.0 - d) * self.gamma * t.cat([self._mlp(c, xa2, False) for c in self.critics_t], 1).min(1).values
        xa = t.cat([s, a], 1)
        loss = sum(F.mse_loss(self._mlp(c, xa, False)[:, 0], y) for c in self.critics)
        self.opt_c.zero_grad(); loss.backward(); self.opt_c.step()
        if self.n % self.delay == 0:
            aloss = -self._mlp(self.critics[0], t.cat([s, self._mlp(self.actor, s, True)], 1), False).mean()
            self.opt_a.zero_grad(); aloss.backward(); self.opt_a.step()
            with t.no_grad():
                for tgt, src in zip([x for c in self.critics_t for x in c] + self.actor_t, [x for c in self.critics for x in c] + self.actor):
                    tgt.mul_(1.0 - self.tau)
                    t.add(tgt, src, alpha=self.tau, out=tgt)


def _passes(n_passes, updates, warmup, step, sync):
    out = []
    for k in range(n_passes + 1):
        n = warmup if k == 0 else updates
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        sync()
        if k:
            out.append((time.perf_counter() - t0) * 1e6 / n)
    return out


def rates(workload, batches, updates, n_passes, with_torch):
    import torch
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.sb3_vec_env import DeviceReplayCollector
    from ev2gym_amd.scenario_gen import generate_native
    from ev2gym_amd.td3 import DDPGLearner, TD3Learner, init_critic_weights
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    lo = 0.0 if kinds[1] == "PublicPST" else -1.0
    D, P = eng.D, eng.P
    actor0 = init_mlp_weights(D, P, 1)
    col = DeviceReplayCollector(eng, actor0, lo=lo, capacity_episodes=2)
    col.collect_episode()
    dev = torch.device("cuda", eng.device)
    sync = lambda: (eng.synchronize(), torch.cuda.synchronize(dev))   # noqa: E731
    for algo, cls in (("td3", TD3Learner), ("ddpg", DDPGLearner)):
        for B in batches:
            learner = cls(col, actor=actor0, seed=3, batch_size=B)
            s, a, r, s2, d = col.sample(B, np.random.default_rng(0))
            r32, d8 = r.to(torch.float32).contiguous(), d.contiguous()
            ring = [(col.obs[b], col.actions[b], col.reward[b], col.done[b]) for b in learner.complete_blocks()]
            bufs = [torch.empty_like(s), torch.empty_like(a), torch.empty_like(r32), torch.empty_like(s2), torch.empty_like(d8)]
            sync()
            counter = [0]

            def sampled():
                eng.replay_sample(ring, col.T, col.E, D, P, B, 3, counter[0], *bufs)
                counter[0] += 1
                eng.td3_update(learner.td3, *bufs, B)

            upd = _passes(n_passes, updates, 20, lambda: eng.td3_update(learner.td3, s, a, r32, s2, d8, B), sync)
            smp = _passes(n_passes, updates, 20, sampled, sync)
            line = dict(workload=workload, algo=algo, batch=B, obs_dim=D, ports=P, updates=updates, passes=n_passes,
                        device_us_per_update=round(statistics.median(upd), 2), device_us_per_update_range=[round(min(upd), 2), round(max(upd), 2)],
                        device_us_per_sampled_update=round(statistics.median(smp), 2), device_us_per_sampled_update_range=[round(min(smp), 2), round(max(smp), 2)])
            if with_torch:
                cfg = learner.cfg
                ref = TorchTD3(actor0, [init_critic_weights(D, P, 4 + j) for j in range(cfg["n_critics"])], dev, lo, cfg["policy_delay"], cfg["target_policy_noise"])
                dd = d8.to(torch.float32)
                tor = _passes(n_passes, updates, 20, lambda: ref.update(s, a, r32, s2, dd), sync)
                line.update(torch_us_per_update=round(statistics.median(tor), 2), torch_us_per_update_range=[round(min(tor), 2), round(max(tor), 2)],
                            torch_over_device=round(statistics.median(tor) / statistics.median(upd), 2))
            print(json.dumps(line), flush=True)
            learner.close()
    col.close()
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--batches", default="100,256,1024")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop")
    args = ap.parse_args()
    for w in args.workloads.split(","):
        rates(w, [int(b) for b in args.batches.split(",")], args.updates, args.passes, not args.no_torch)
