#!/usr/bin/env python3
"""EV-free stretches of a scenario pool, per workgroup of the fast-path step kernel (development tool; numpy only, no GPU).
A step is EV-free for an env when no port holds an EV during it and none receives one at its end: no session with t_arr - 1 <= t <= t_dep.
A workgroup-step is EV-free when it is for all of the workgroup's (four consecutive) envs.
  python tools/ev_free_stretches.py [cfg2|cfg3] [envs] [windows] [n_min]
prints, for the first `windows` windows of the benchmark's pool (seed 0, sorted by busy window like bench.py): the share of EV-free
workgroup-steps, the live steps of the busiest workgroup, and what a persistent whole-episode launch fast-forwards (stretches of at least
n_min steps, the launch's last step excluded)."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def env_free(batch):
    """[E, T] bool: step t of env e is EV-free."""
    E, T = batch.n_envs, batch.n_steps
    st, ta, td = batch.arrays["env_session_start"], batch.arrays["ev_t_arr"], batch.arrays["ev_t_dep"]
    d = np.zeros((E, T + 1), np.int64)
    env_of = np.repeat(np.arange(E), np.diff(st))
    lo, hi = np.clip(ta - 1, 0, T), np.clip(td + 1, 0, T)
    ok = hi > lo
    np.add.at(d, (env_of[ok], lo[ok]), 1)
    np.add.at(d, (env_of[ok], hi[ok]), -1)
    return np.cumsum(d, axis=1)[:, :T] == 0


def group_free(free, envs_per_group=4):
    E, T = free.shape
    pad = (-E) % envs_per_group
    f = np.concatenate([free, np.ones((pad, T), bool)]) if pad else free
    return f.reshape(-1, envs_per_group, T).all(axis=1)


def fast_forwarded(gfree, t0, k, n_min=1):
    """(steps, stretches) a launch of steps t0 .. t0 + k - 1 fast-forwards: per workgroup, maximal runs of EV-free steps among the launch's
    steps but its last, in chunks as the kernel finds them (a run is found whole: the kernel looks ahead to the next live step)."""
    steps = stretches = 0
    if k < 2:
        return 0, 0
    for row in gfree[:, t0:t0 + k - 1]:
        t = 0
        while t < len(row):
            if not row[t]:
                t += 1
                continue
            n = 1
            while n < 64 and t + n < len(row) and row[t + n]:   # (one pass of the kernel covers at most 64 steps)
                n += 1
            if n >= n_min:
                steps += n; stretches += 1
            t += n
    return steps, stretches


def main():
    from bench import WORKLOADS
    from ev2gym_amd.scenario_gen import generate_native
    a = sys.argv[1:]
    wname = a[0] if a else "cfg2"
    wl = WORKLOADS[wname]
    E = int(a[1]) if len(a) > 1 else wl["envs"]
    W = int(a[2]) if len(a) > 2 else 2
    n_min = int(a[3]) if len(a) > 3 else 1
    batch = generate_native(wl["gen"](E * 8, 0)).sorted_by_busy_window(E)
    T = batch.n_steps
    for w in range(W):
        gf = group_free(env_free(batch.select(np.arange(w * E, (w + 1) * E))))
        live = T - gf.sum(axis=1)
        s, n = fast_forwarded(gf, 0, T, n_min)
        print(f"{wname} window {w}: {gf.shape[0]} workgroups x {T} steps; EV-free workgroup-steps {gf.mean() * 100:.1f} %; live steps per workgroup "
              f"min {live.min()} mean {live.mean():.1f} p99 {np.percentile(live, 99):.0f} max {live.max()} (EV-free steps of that workgroup: {T - live.max()}); "
              f"fast-forwarded by a whole-episode launch (n_min {n_min}): {s} workgroup-steps in {n} stretches")


if __name__ == "__main__":
    main()
