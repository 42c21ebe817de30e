#!/usr/bin/env python3
"""Length of a persistent whole-episode launch when the price of a live step depends on how many workgroups its CU still holds (development
tool; numpy only, no GPU).
A workgroup of the fast-path kernel steps its live steps one after the other (EV-free stretches are fast-forwarded: tools/ev_free_stretches.py)
and leaves its CU when it is done; a live step costs price[r] with r workgroups resident on the CU (profiles/r25_cu_balance.txt, 0.1).
The measurement (0.3 there) ranks the two re-orderings the other way round than this model does: it is kept as the record of what was predicted.
A CU that holds workgroups of L_1 <= .. <= L_n live steps is then busy for  sum_i (L_i - L_(i-1)) * price[n - i + 1],  and the launch is as long
as its busiest CU.  Units: live steps at the four-resident price.
  python tools/cu_balance_model.py [cfg2] [envs] [windows] [p4,p3,p2,p1] [placement.json]
prints, for the first `windows` windows of the benchmark's pool, the launch length under today's workgroup -> env-group map and under two
re-orderings of the groups (snake over the CUs; every CU one of the heaviest groups and the lightest ones left), for a placement file written
by tools/cu_balance_probe.py (blockIdx.x -> CU as observed) or, without one, for the two textbook policies inside an XCD."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRICES = (1.000, 0.905, 0.827, 0.775)   # 4, 3, 2, 1 resident workgroups (profiles/r25_cu_balance.txt, 0.1)


def xcd_map(nb):
    """env group of workgroup b (ev2g_step_wave.h: each XCD a contiguous range of groups)."""
    b = np.arange(nb)
    return (b & 7) * (nb >> 3) + (b >> 3) if nb % 8 == 0 else b


def textbook_placement(nb, policy, n_cu=256, per_cu=4):
    """CU of workgroup b when block b runs on XCD b % 8 and an XCD deals its blocks to its CUs round-robin or fills one CU after the other."""
    b = np.arange(nb)
    x, j = b & 7, b >> 3
    cpx = n_cu // 8
    return x * cpx + (j % cpx if policy == "round-robin" else (j // per_cu) % cpx)


def cu_time(live, price):
    """Busy time of one CU holding workgroups of `live` live steps (price[r - 1] = cost of a live step with r resident; more than len(price): the last)."""
    L = np.sort(np.asarray(live, np.float64))
    n, t, prev = len(L), 0.0, 0.0
    for i, x in enumerate(L):
        r = n - i
        t += (x - prev) * price[min(r, len(price)) - 1]
        prev = x
    return t


def launch_length(group_live, cu_of_block, block_group, price):
    """max over the CUs; group_live[g], cu_of_block[b], block_group[b] = the env group workgroup b steps."""
    out = 0.0
    for c in np.unique(cu_of_block):
        out = max(out, cu_time(group_live[block_group[cu_of_block == c]], price))
    return out


def balanced_order(group_live, cu_of_block, block_group, how):
    """src[g] = the group whose scenarios should stand in group g's place so that, under this placement, the CUs get
    `heavy+light`: one of the heaviest groups each, the heaviest of them the lightest ones left;  `snake`: the groups dealt heaviest first, forth and back."""
    cus, inv = np.unique(cu_of_block, return_inverse=True)
    slots = [list(np.flatnonzero(inv == i)) for i in range(len(cus))]   # blocks of every CU
    order = np.argsort(-group_live, kind="stable")   # heaviest first
    src = np.empty(len(group_live), np.int64)
    if how == "snake":
        k, rnd = 0, 0
        while k < len(order):
            seq = [i for i in range(len(cus)) if len(slots[i]) > rnd]
            for i in (seq if rnd % 2 == 0 else seq[::-1]):
                src[block_group[slots[i][rnd]]] = order[k]; k += 1
            rnd += 1
        return src
    n_cu = len(cus)
    for i in range(n_cu):   # CU i takes the i-th heaviest group ...
        src[block_group[slots[i][0]]] = order[i]
    light = list(order[n_cu:][::-1])   # ... and, in that order, the lightest groups left for its other workgroups
    for i in range(n_cu):
        for b in slots[i][1:]:
            src[block_group[b]] = light.pop(0)
    return src


def pool_group_live(wname, E, W):
    from bench import WORKLOADS
    from ev2gym_amd.scenario_gen import generate_native
    from tools.ev_free_stretches import env_free, group_free
    wl = WORKLOADS[wname]
    batch = generate_native(wl["gen"](wl["envs"] * 8, 0)).sorted_by_busy_window(wl["envs"])
    T = batch.n_steps
    return [T - group_free(env_free(batch.select(np.arange(w * wl["envs"], w * wl["envs"] + E)))).sum(axis=1) for w in range(W)]


def main():
    a = sys.argv[1:]
    wname = a[0] if a else "cfg2"
    E = int(a[1]) if len(a) > 1 else 4096
    W = int(a[2]) if len(a) > 2 else 4
    price = tuple(float(x) for x in a[3].split(","))[::-1] if len(a) > 3 else PRICES[::-1]   # -> price[r - 1]
    placements = {}
    nb = (E + 3) // 4
    if len(a) > 4:
        placements["observed"] = np.asarray(json.load(open(a[4]))["cu_of_block"])
    else:
        placements = {p: textbook_placement(nb, p) for p in ("round-robin", "fill-first")}
    bg = xcd_map(nb)
    print(f"{wname}, {E} envs = {nb} workgroups; price of a live step at 1 / 2 / 3 / 4 resident workgroups: {' / '.join(f'{p:.3f}' for p in price)}")
    for w, live in enumerate(pool_group_live(wname, E, W)):
        for name, cu in placements.items():
            today = launch_length(live, cu, bg, price)
            row = [f"window {w} ({name}): busiest workgroup {live.max()} live steps, mean {live.mean():.1f}; today's map {today:.1f}"]
            for how in ("snake", "heavy+light"):
                src = balanced_order(live, cu, bg, how)
                x = launch_length(live[src], cu, bg, price)
                row.append(f"{how} {x:.1f} ({(x / today - 1) * 100:+.1f} %)")
            print("; ".join(row))


if __name__ == "__main__":
    main()
