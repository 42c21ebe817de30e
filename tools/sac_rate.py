"""Wall clock of one SAC update on the device (ev2g_sac_update, with and without the device sampler ev2g_replay_sample in front of it) next to
the same batch through a torch-on-GPU module set with autograd and three torch.optim.Adam(eps=1e-8); and of one collected step of
ev2g_sac_collect next to ev2g_collect's unfused loop with a deterministic policy of the same widths on the same engine.  One JSON line per
(workload, batch size), one per workload for the collection.

  python tools/sac_rate.py [--workloads cfg2,cfg3] [--batches 256,1024] [--updates 200] [--passes 3] [--no-torch] [--no-collect]
      microseconds per update: medians over --passes passes of --updates updates after a warm-up of 20, each pass ended by ONE synchronisation (the
      updates of a pass are queued back to back, as SACLearner.train() queues them).  The replay ring is one collected episode of the workload.
      microseconds per collected step: whole episodes, medians over --passes episodes after one warm-up episode.
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/sac_rate.py --workloads cfg2 --batches 256 --updates 50 --passes 1 --no-torch --no-collect
      kernel time of an update: the ev2g_sac_*, ev2g_td3_* and ev2g_replay_sample_kernel rows of OUT's kernel statistics

The workloads are bench.py's shapes (tools/heuristic_rate.py WORKLOADS) with SB3's 256-256 SAC networks.  There is no rate threshold: the figures
time the arithmetic, not learning."""
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
from td3_rate import _passes  # noqa: E402

HALF_LOG_2PI = 0.9189385332046727


class TorchSAC:
    """SB3's SACPolicy (256-256 ReLU squashed-Gaussian actor, n critics) and SAC.train()'s gradient step in torch on the GPU."""

    def __init__(self, actor, critics, dev, lo, lr=3e-4, tau=0.005, gamma=0.99):
        import torch
        self.torch, self.lo, self.tau, self.gamma = torch, lo, tau, gamma
        mk = lambda ws, grad: [torch.from_numpy(np.array(a)).to(dev).requires_grad_(grad) for a in ws]  # noqa: E731
        self.actor, self.critics, self.critics_t = mk(actor, True), [mk(c, True) for c in critics], [mk(c, False) for c in critics]
        self.la = torch.zeros(1, device=dev, requires_grad=True)
        self.te = -float(actor[4].shape[0])
        self.opt_a = torch.optim.Adam(self.actor, lr=lr, eps=1e-8)
        self.opt_c = torch.optim.Adam([a for c in self.critics for a in c], lr=lr, eps=1e-8)
        self.opt_e = torch.optim.Adam([self.la], lr=lr, eps=1e-8)

    def _mlp(self, w, x):
        t = self.torch
        F = t.nn.functional
        return F.linear(t.relu(F.linear(t.relu(F.linear(x, w[0], w[1])), w[2], w[3])), w[4], w[5])

    def _pi(self, s):
        t = self.torch
        F = t.nn.functional
        w = self.actor
        h = t.relu(F.linear(t.relu(F.linear(s, w[0], w[1])), w[2], w[3]))
        mu, ls = F.linear(h, w[4], w[5]), t.clamp(F.linear(h, w[6], w[7]), -20.0, 2.0)
        eps = t.randn_like(mu)
        a = t.tanh(mu + ls.exp() * eps)
        return a, (-0.5 * eps * eps - ls - HALF_LOG_2PI).sum(1) - t.log(1.0 - a * a + 1e-6).sum(1)

    def update(self, s, a, r, s2, d):
        t = self.torch
        F = t.nn.functional
        if self.lo == 0.0:
            a = 2.0 * a - 1.0
        a_pi, lp = self._pi(s)
        alpha = self.la.detach().exp()
        eloss = -(self.la * (lp.detach() + self.te)).mean()
        self.opt_e.zero_grad(); eloss.backward(); self.opt_e.step()
        with t.no_grad():
            a2, lp2 = self._pi(s2)
            tq = t.cat([self._mlp(c, t.cat([s2, a2], 1)) for c in self.critics_t], 1).min(1).values
            y = r + (1.0 - d) * self.gamma * (tq - alpha * lp2)
        xa = t.cat([s, a], 1)
        closs = 0.5 * sum(F.mse_loss(self._mlp(c, xa)[:, 0], y) for c in self.critics)
        self.opt_c.zero_grad(); closs.backward(); self.opt_c.step()
        q = t.cat([self._mlp(c, t.cat([s, a_pi], 1)) for c in self.critics], 1).min(1).values
        aloss = (alpha * lp - q).mean()
        self.opt_a.zero_grad(); aloss.backward(); self.opt_a.step()
        with t.no_grad():
            for tgt, src in zip([x for c in self.critics_t for x in c], [x for c in self.critics for x in c]):
                tgt.mul_(1.0 - self.tau)
                t.add(tgt, src, alpha=self.tau, out=tgt)


def rates(workload, batches, updates, n_passes, with_torch, with_collect):
    import torch
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.sac import SACCollector, SACLearner, init_sac_actor_weights
    from ev2gym_amd.sb3_vec_env import DeviceReplayCollector
    from ev2gym_amd.scenario_gen import generate_native
    from ev2gym_amd.td3 import init_critic_weights
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    lo = 0.0 if kinds[1] == "PublicPST" else -1.0
    D, P = eng.D, eng.P
    actor0 = init_sac_actor_weights(D, P, 1)
    col = SACCollector(eng, actor0, lo=lo, capacity_episodes=2)
    dev = torch.device("cuda", eng.device)
    sync = lambda: (eng.synchronize(), torch.cuda.synchronize(dev))   # noqa: E731
    first = True
    for B in batches:
        learner = SACLearner(col, actor=actor0, seed=3, batch_size=B)
        if first:
            col.collect_episode()
            first = False
        s, a, r, s2, d = col.sample(B, np.random.default_rng(0))
        r32, d8 = r.to(torch.float32).contiguous(), d.contiguous()
        ring = [(col.obs[b], col.actions[b], col.reward[b], col.done[b]) for b in learner.complete_blocks()]
        bufs = [torch.empty_like(s), torch.empty_like(a), torch.empty_like(r32), torch.empty_like(s2), torch.empty_like(d8)]
        sync()
        counter = [0]

        def sampled():
            eng.replay_sample(ring, col.T, col.E, D, P, B, 3, counter[0], *bufs)
            counter[0] += 1
            eng.sac_update(learner.sac, *bufs, B)

        upd = _passes(n_passes, updates, 20, lambda: eng.sac_update(learner.sac, s, a, r32, s2, d8, B), sync)
        smp = _passes(n_passes, updates, 20, sampled, sync)
        line = dict(workload=workload, algo="sac", batch=B, obs_dim=D, ports=P, updates=updates, passes=n_passes,
                    device_us_per_update=round(statistics.median(upd), 2), device_us_per_update_range=[round(min(upd), 2), round(max(upd), 2)],
                    device_us_per_sampled_update=round(statistics.median(smp), 2), device_us_per_sampled_update_range=[round(min(smp), 2), round(max(smp), 2)])
        if with_torch:
            ref = TorchSAC(actor0, [init_critic_weights(D, P, 4 + j, 256, 256) for j in range(2)], dev, lo)
            dd = d8.to(torch.float32)
            tor = _passes(n_passes, updates, 20, lambda: ref.update(s, a, r32, s2, dd), sync)
            line.update(torch_us_per_update=round(statistics.median(tor), 2), torch_us_per_update_range=[round(min(tor), 2), round(max(tor), 2)],
                        torch_over_device=round(statistics.median(tor) / statistics.median(upd), 2))
        print(json.dumps(line), flush=True)
        if B != batches[-1] or not with_collect:
            learner.close()
    if with_collect:   # one collected step: the stochastic SAC actor against the deterministic policy of the same widths, both unfused
        if not batches:
            SACLearner(col, actor=actor0, seed=3)
        T = col.T

        def episodes(collect):
            out = []
            for k in range(n_passes + 1):
                sync()
                t0 = time.perf_counter()
                collect()
                sync()
                if k:
                    out.append((time.perf_counter() - t0) * 1e6 / T)
            return out

        sac_us = episodes(col.collect_episode)
        col.close()
        det = DeviceReplayCollector(eng, init_mlp_weights(D, P, 1, 256, 256), lo=lo, capacity_episodes=2, precision="fp32")
        os.environ["EV2G_NO_FUSED"] = "1"   # (ev2g_collect's loop: actor launch -> step launch, as ev2g_sac_collect runs)
        det_us = episodes(det.collect_episode)
        del os.environ["EV2G_NO_FUSED"]
        print(json.dumps(dict(workload=workload, collect="per step", envs=eng.E, obs_dim=D, ports=P, steps_per_episode=T, passes=n_passes,
                              sac_collect_us_per_step=round(statistics.median(sac_us), 2), sac_collect_us_per_step_range=[round(min(sac_us), 2), round(max(sac_us), 2)],
                              deterministic_collect_us_per_step=round(statistics.median(det_us), 2),
                              deterministic_collect_us_per_step_range=[round(min(det_us), 2), round(max(det_us), 2)], deterministic_policy_kernel=eng.mlp_kernel_name(det.mlp),
                              sac_over_deterministic=round(statistics.median(sac_us) / statistics.median(det_us), 2))), flush=True)
        det.close()
    else:
        col.close()
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop")
    ap.add_argument("--no-collect", action="store_true", help="skip the collection timing")
    args = ap.parse_args()
    for w in args.workloads.split(","):
        rates(w, [int(b) for b in args.batches.split(",") if b], args.updates, args.passes, not args.no_torch, not args.no_collect)
