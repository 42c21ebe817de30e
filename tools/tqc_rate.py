"""Wall clock of one TQC update on the device (ev2g_tqc_update, with and without the device sampler ev2g_replay_sample in front of it) next to
the same batch through a torch-on-GPU module set with autograd, torch.sort and three torch.optim.Adam(eps=1e-8); and -- the SAC learner shares its
actor side, its optimiser steps and its read-backs with this one -- ev2g_sac_update of this tree next to ev2g_sac_update of a checkout of the
parent commit on the same device, alternating.  One JSON line per (workload, batch size), one per workload for the SAC comparison.

  python tools/tqc_rate.py [--workloads cfg2,cfg3] [--batches 256,1024] [--updates 100] [--passes 3] [--no-torch] [--sac-parent DIR] [--rounds 3]
      microseconds per update: medians over --passes passes of --updates updates after a warm-up of 20, each pass ended by ONE synchronisation (the
      updates of a pass are queued back to back, as TQCLearner.train() queues them).  The replay ring is one collected episode of the workload.
      --sac-parent DIR: a checkout of the parent commit with its library built (DIR/tools/sac_rate.py, DIR/ev2gym_amd/libev2g_hip.so).  Each of
      --rounds rounds runs that tree's tools/sac_rate.py and then this tree's in a fresh process each (--no-torch --no-collect, the same
      arguments); the line holds the medians over the rounds and each round's pair.
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/tqc_rate.py --workloads cfg2 --batches 256 --updates 50 --passes 1 --no-torch
      kernel time of an update: the ev2g_tqc_*, ev2g_sac_*, ev2g_td3_* and ev2g_replay_sample_kernel rows of OUT's kernel statistics

The workloads are bench.py's shapes (tools/heuristic_rate.py WORKLOADS) with 256-256 networks and sb3_contrib's 2 x 25 quantiles, 2 dropped per
net.  There is no rate threshold: the figures time the arithmetic, not learning."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from ev2gym_amd import _abi  # noqa: E402
from heuristic_rate import WORKLOADS  # noqa: E402
from sac_rate import TorchSAC  # noqa: E402
from td3_rate import _passes  # noqa: E402


class TorchTQC(TorchSAC):
    """sb3_contrib's TQCPolicy (SAC's actor, n quantile critics) and TQC.train()'s gradient step in torch on the GPU."""

    def __init__(self, actor, critics, dev, lo, drop=2, **kw):
        super().__init__(actor, critics, dev, lo, **kw)
        self.nq = critics[0][4].shape[0]
        self.K = len(critics) * (self.nq - drop)
        self.cum_prob = ((self.torch.arange(self.nq, device=dev, dtype=self.torch.float32) + 0.5) / self.nq).view(1, 1, -1, 1)

    def update(self, s, a, r, s2, d):
        t = self.torch
        if self.lo == 0.0:
            a = 2.0 * a - 1.0
        a_pi, lp = self._pi(s)
        alpha = self.la.detach().exp()
        eloss = -(self.la * (lp.detach() + self.te)).mean()
        self.opt_e.zero_grad(); eloss.backward(); self.opt_e.step()
        with t.no_grad():
            a2, lp2 = self._pi(s2)
            xn = t.cat([s2, a2], 1)
            pooled = t.stack([self._mlp(c, xn) for c in self.critics_t], 1).reshape(s.shape[0], -1)
            z = t.sort(pooled, dim=1).values[:, :self.K]
            z = r[:, None] + (1.0 - d)[:, None] * self.gamma * (z - alpha * lp2[:, None])
        xa = t.cat([s, a], 1)
        cur = t.stack([self._mlp(c, xa) for c in self.critics], 1)
        delta = z[:, None, None, :] - cur[:, :, :, None]
        ad = delta.abs()
        closs = (t.abs(self.cum_prob - (delta.detach() < 0).float()) * t.where(ad > 1.0, ad - 0.5, delta ** 2 * 0.5)).mean()
        self.opt_c.zero_grad(); closs.backward(); self.opt_c.step()
        xp = t.cat([s, a_pi], 1)
        qf_pi = t.stack([self._mlp(c, xp) for c in self.critics], 1).mean(dim=2).mean(dim=1)
        aloss = (alpha * lp - qf_pi).mean()
        self.opt_a.zero_grad(); aloss.backward(); self.opt_a.step()
        with t.no_grad():
            for tgt, src in zip([x for c in self.critics_t for x in c], [x for c in self.critics for x in c]):
                tgt.mul_(1.0 - self.tau)
                t.add(tgt, src, alpha=self.tau, out=tgt)


def rates(workload, batches, updates, n_passes, with_torch, nc=2, nq=25, drop=2):
    import torch
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.sac import init_sac_actor_weights
    from ev2gym_amd.scenario_gen import generate_native
    from ev2gym_amd.tqc import TQCCollector, TQCLearner, init_tqc_critic_weights
    E, gen, kinds = WORKLOADS[workload]
    eng = Engine(generate_native(gen(E, 1234)), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], flags=_abi.FLAG_LOG_SOC)
    lo = 0.0 if kinds[1] == "PublicPST" else -1.0
    D, P = eng.D, eng.P
    actor0 = init_sac_actor_weights(D, P, 1)
    col = TQCCollector(eng, actor0, lo=lo, capacity_episodes=2)
    dev = torch.device("cuda", eng.device)
    sync = lambda: (eng.synchronize(), torch.cuda.synchronize(dev))   # noqa: E731
    first = True
    for B in batches:
        learner = TQCLearner(col, actor=actor0, seed=3, batch_size=B, n_critics=nc, n_quantiles=nq, top_quantiles_to_drop_per_net=drop)
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
            eng.tqc_update(learner.tqc, *bufs, B)

        upd = _passes(n_passes, updates, 20, lambda: eng.tqc_update(learner.tqc, s, a, r32, s2, d8, B), sync)
        smp = _passes(n_passes, updates, 20, sampled, sync)
        line = dict(workload=workload, algo="tqc", batch=B, obs_dim=D, ports=P, n_critics=nc, n_quantiles=nq, drop=drop, updates=updates, passes=n_passes,
                    device_us_per_update=round(statistics.median(upd), 2), device_us_per_update_range=[round(min(upd), 2), round(max(upd), 2)],
                    device_us_per_sampled_update=round(statistics.median(smp), 2), device_us_per_sampled_update_range=[round(min(smp), 2), round(max(smp), 2)])
        if with_torch:
            ref = TorchTQC(actor0, [init_tqc_critic_weights(D, P, nq, 4 + j, 256, 256) for j in range(nc)], dev, lo, drop)
            dd = d8.to(torch.float32)
            tor = _passes(n_passes, updates, 20, lambda: ref.update(s, a, r32, s2, dd), sync)
            line.update(torch_us_per_update=round(statistics.median(tor), 2), torch_us_per_update_range=[round(min(tor), 2), round(max(tor), 2)],
                        torch_over_device=round(statistics.median(tor) / statistics.median(upd), 2))
        print(json.dumps(line), flush=True)
        learner.close()
    col.close()
    eng.close()


def sac_against_parent(parent, workload, batches, updates, n_passes, rounds):
    """ev2g_sac_update of the parent commit's tree and of this one, alternating, a fresh process each: per batch size the medians over the rounds."""
    args = ["--workloads", workload, "--batches", ",".join(str(b) for b in batches), "--updates", str(updates), "--passes", str(n_passes), "--no-torch", "--no-collect"]
    got = {"parent": {B: [] for B in batches}, "this": {B: [] for B in batches}}
    for _ in range(rounds):
        for side, tree in (("parent", parent), ("this", ROOT)):
            env = {k: v for k, v in os.environ.items() if k != "EV2G_LIB"}
            out = subprocess.run([sys.executable, os.path.join(tree, "tools", "sac_rate.py"), *args], cwd=tree, env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError(f"tools/sac_rate.py of {tree} failed: {out.stderr[-2000:]}")
            for ln in out.stdout.splitlines():
                if ln.startswith("{"):
                    rec = json.loads(ln)
                    got[side][rec["batch"]].append(rec["device_us_per_update"])
    for B in batches:
        p, t = got["parent"][B], got["this"][B]
        print(json.dumps(dict(workload=workload, algo="sac", batch=B, rounds=rounds, updates=updates, passes=n_passes, parent_us_per_update=round(statistics.median(p), 2),
                              this_us_per_update=round(statistics.median(t), 2), this_over_parent=round(statistics.median(t) / statistics.median(p), 3),
                              parent_rounds=p, this_rounds=t)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg2,cfg3")
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop")
    ap.add_argument("--no-tqc", action="store_true", help="skip the TQC timing (with --sac-parent: the SAC comparison alone)")
    ap.add_argument("--sac-parent", default=None, help="a checkout of the parent commit with its library built: time its ev2g_sac_update against this tree's")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",") if b]
    for w in args.workloads.split(","):
        if not args.no_tqc:
            rates(w, batches, args.updates, args.passes, not args.no_torch)
        if args.sac_parent:
            sac_against_parent(os.path.abspath(args.sac_parent), w, batches, args.updates, args.passes, args.rounds)
