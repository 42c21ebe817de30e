#!/usr/bin/env python3
"""Does it pay to put a persistent launch's busiest workgroups on a CU with its lightest ones?  (development probe, one MI355X; the model is
tools/cu_balance_model.py, the record profiles/r25_cu_balance.txt.)
  python tools/cu_balance_probe.py [out_dir]
1. the launch time per live step of the busiest workgroup at 4096 / 3072 / 2048 / 1024 envs (4 / 3 / 2 / 1 workgroups per CU if the hardware spreads them
   evenly) -- whole-episode persistent launches over the first four windows of the benchmark's pool, the first E scenarios of each, HIP events;
2. where the workgroups of those launches ran (EV2G_PLACEMENT=1, ev2g_last_launch_placement), over ten launches;
3. the benchmark's launch with the scenarios of every window re-ordered so that, under the placement of item 2, every CU gets one of the heaviest
   groups and the lightest ones left (and dealt as a snake), against the benchmark's order, alternating; next to it what the model predicts."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ev2gym_amd import _abi
from ev2gym_amd.engine import Engine
from ev2gym_amd.scenario_gen import generate_native
from bench import WORKLOADS
from tools.ev_free_stretches import env_free, group_free
from tools import cu_balance_model as model

W, E0 = 4, 4096
wl = WORKLOADS["cfg2"]
rk, sk = _abi.REWARD_KINDS[wl["reward"]], _abi.STATE_KINDS[wl["state"]]


class Run:
    """An engine over W windows of E scenarios each, with the benchmark's buffers; episodes = persistent launch + statistics and reset in one launch."""

    def __init__(self, batch, E, placement=False):
        os.environ.pop("EV2G_PLACEMENT", None)
        if placement:
            os.environ["EV2G_PLACEMENT"] = "1"
        self.eng = eng = Engine(batch, rk, sk, flags=_abi.FLAG_LOG_SOC, n_active_envs=E)
        os.environ.pop("EV2G_PLACEMENT", None)
        self.E, self.P, self.T = E, eng.P, eng.T
        self.acts = eng.empty((eng.T, E, eng.P)); eng.fill_uniform(self.acts, eng.T * E * eng.P, 999, wl["lo"], 1.0)
        self.obs, self.rew, self.done, self.mask = eng.empty((E, eng.D)), eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, eng.P), np.uint8)
        self.stats = eng.empty((E, _abi.N_STATS))
        self.w = 0
        eng.reset(self.obs, offset=0)

    def episode(self):
        """-> the window the launch stepped"""
        e, w = self.eng, self.w
        e.step_n(self.T, self.acts, self.E * self.P, self.obs, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=True)
        self.w = (w + 1) % W
        e.stats_reset(self.stats, self.obs, offset=self.w * self.E)
        return w

    def timed(self, rounds):
        """[rounds, W] launch time in us (HIP events), `rounds` passes over the windows queued back to back"""
        assert self.w == 0 and rounds * W <= 32
        for _ in range(rounds * W):
            self.episode()
        self.eng.synchronize()
        n = rounds * W
        return np.array([self.eng.step_n_kernel_ms_back(n - 1 - i) * 1e3 for i in range(n)]).reshape(rounds, W)

    def close(self):
        self.eng.check_faults(); self.eng.close()


def cu_ids(pl):
    """dense CU index per workgroup from the reporter's words (XCC, and SE | SH | CU of HW_REG_HW_ID)"""
    key = ((pl[:, 0] >> 16) << 8) | ((pl[:, 0] >> 8) & 0xff)
    return np.unique(key, return_inverse=True)[1], key


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    pool = generate_native(wl["gen"](E0 * 8, 0)).sorted_by_busy_window(E0)
    T = pool.n_steps
    sub = lambda E: pool.select(np.concatenate([w * E0 + np.arange(E) for w in range(W)]))
    live_of = lambda b, E: [T - group_free(env_free(b.select(np.arange(w * E, (w + 1) * E)))).sum(axis=1) for w in range(W)]

    print("== 1 + 2: launch time per live step of the busiest workgroup, and where the workgroups ran ==", flush=True)
    price, place0 = {}, None
    for E in (4096, 3072, 2048, 1024):
        b = sub(E)
        live = live_of(b, E)
        r = Run(b, E)
        r.timed(1)
        us = np.median(np.concatenate([r.timed(4), r.timed(4)]), axis=0)
        r.close()
        lmax = np.array([l.max() for l in live])
        q = us / lmax
        price[E] = float(np.mean(q))
        print(f"{E} envs ({(E + 3) // 4} workgroups): launch us per window {np.round(us, 1).tolist()}; busiest workgroup {lmax.tolist()} live steps (mean {np.mean([l.mean() for l in live]):.1f}); "
              f"us per live step of it {np.round(q, 3).tolist()} mean {price[E]:.3f}", flush=True)
        r = Run(b, E, placement=True)
        seen = []
        for i in range(10):
            r.eng.step_n(r.T, r.acts, E * r.P, r.obs, 0, r.rew, 0, r.done, 0, r.mask, 0, auto_reset=False, persistent=True)
            seen.append((i % W, r.eng.last_launch_placement().copy()))   # (read between the launch and the episode's end: the reporter speaks of the LAST launch)
            r.eng.stats_reset(r.stats, r.obs, offset=((i + 1) % W) * E)
        r.close()
        cu, key = cu_ids(seen[0][1])
        per_cu = np.bincount(cu)
        nb = len(cu)
        xcc = seen[0][1][:, 0] >> 16
        same_xcd = all(len(np.unique(xcc[x::8])) == 1 for x in range(8)) if nb % 8 == 0 else None
        stable = [float(np.mean(cu_ids(p)[1] == key)) for _, p in seen[1:]]
        ranks = seen[0][1][:, 1]
        print(f"   placement, launch 0: {len(per_cu)} CUs used, workgroups per CU {dict(zip(*np.unique(per_cu, return_counts=True)))}; XCDs used {len(np.unique(xcc))}, "
              f"blocks b, b + 8 on one XCD: {same_xcd}; arrival ranks {dict(zip(*np.unique(ranks, return_counts=True)))}; "
              f"share of workgroups on the same CU as in launch 0, later launches: {np.round(stable, 3).tolist()}", flush=True)
        x0 = np.flatnonzero((np.arange(nb) & 7) == 0)[:40]
        print(f"   CU (SE|SH|CU bits) of blocks 0, 8, 16, ..: {[hex(int(k) & 0xff) for k in key[x0]]}", flush=True)
        if E == E0:
            place0 = cu
            json.dump({"envs": E, "cu_of_block": cu.tolist(), "hw_words": seen[0][1][:, 0].tolist(), "rank": ranks.tolist(),
                       "later_launches_same_cu_share": stable}, open(os.path.join(out_dir, "r25_placement.json"), "w"))
    p4 = price[4096]
    rel = [price[e] / p4 for e in (4096, 3072, 2048, 1024)]
    print(f"price of a live step at 4 / 3 / 2 / 1 workgroups per CU, relative: {' / '.join(f'{x:.3f}' for x in rel)}", flush=True)

    print("== 3: the benchmark's order against the re-ordered windows, under the placement of launch 0 ==", flush=True)
    b = sub(E0)
    live = live_of(b, E0)
    nb = E0 // 4
    bg = model.xcd_map(nb)
    variants = {"bench": b}
    for how in ("heavy+light", "snake"):
        perm = []
        for w in range(W):
            src = model.balanced_order(live[w], place0, bg, how)
            perm.append(w * E0 + (4 * src[:, None] + np.arange(4)[None, :]).reshape(-1))
            pr = rel[::-1]
            print(f"   model, window {w}, {how}: today's map {model.launch_length(live[w], place0, bg, pr):.1f} -> {model.launch_length(live[w][src], place0, bg, pr):.1f} "
                  f"live steps at the four-resident price (busiest workgroup {live[w].max()})", flush=True)
        variants[how] = b.select(np.concatenate(perm))
    runs = {k: Run(v, E0) for k, v in variants.items()}
    for r in runs.values():
        r.timed(1)
    series = {k: [] for k in runs}
    for rnd in range(5):
        for k, r in runs.items():
            series[k].append(r.timed(4))
    for k, r in runs.items():
        r.close()
    base = None
    for k, s in series.items():
        per_round = [float(np.median(x)) for x in s]
        per_window = np.median(np.concatenate(s), axis=0)
        med = float(np.median(np.concatenate(s)))
        base = base or med
        print(f"{k:12s} launch us: median of each alternating round {np.round(per_round, 1).tolist()}; per window {np.round(per_window, 1).tolist()}; "
              f"median {med:.1f} ({(med / base - 1) * 100:+.2f} % against the benchmark's order)", flush=True)


if __name__ == "__main__":
    main()
