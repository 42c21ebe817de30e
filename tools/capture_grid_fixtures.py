"""Records the grid fixtures tests/golden/grid/grid_<n_bus>.npz from the reference's own power-flow code (CPU, run once where a checkout of
the reference exists; oracle/ref_import.py makes it importable and stands in for the modules it imports but does not need here).

Per network (the reference's 34-bus and 123-bus feeders) a fixture holds
  K, L, pf          GridTensor's matrices and power factors
  P, Q              [cases, n] node powers in kW: the nominal loads scaled by a seeded factor in 0.3 .. 3 plus EV injections in -22 .. 22 kW per bus
  v, vm, iters      GridTensor.run_pf on each row alone (ts = 1): complex voltages, |v| with the slack in front, iteration count
  res               [cases, 2] the last two residuals, from run_pf_tensor stopped after iters - 1 and iters - 2 iterations
  traj_*            a 3-step PowerGrid.reset / step trajectory on seeded load / PV profiles (PowerGrid is built without __init__, which wants the
                    load generator's pickle that the reference's repository does not ship)
and the network's two CSV files are copied next to it (data, read by GridNetwork.from_files in the tests).

Iteration-count guard: a case whose final residual, or the one before it, lies within a relative 1e-3 of the tolerance is NOT written -- its
count could flip on rounding.  Cases are kept in an order that puts different counts next to each other.

    python tools/capture_grid_fixtures.py
"""
import datetime
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "grid")
TOL, GUARD = 1e-6, 1e-3
N_CASES = 16
NETWORKS = ((34, "node_34/Nodes_34.csv", "node_34/Lines_34.csv", 340), (123, "node_123/Nodes_123.csv", "node_123/Lines_123.csv", 1230))


def residual(net, P, Q, k):
    """max | |v_k| - |v_(k-1)| | of one row, both from the reference's solver run for exactly k and k - 1 iterations (tolerance 0)."""
    if k < 1:
        return np.inf
    a = net.run_pf_tensor(P.copy(), Q.copy(), iterations=k, tolerance=0.0)["v"]
    b = net.run_pf_tensor(P.copy(), Q.copy(), iterations=k - 1, tolerance=0.0)["v"] if k > 1 else np.ones_like(a)
    return float(np.max(np.abs(np.abs(a) - np.abs(b))))


def near(x):
    return abs(x - TOL) <= GUARD * TOL


def capture(n_bus, bus_csv, branch_csv, seed):
    from ev2gym.models.grid import PowerGrid
    from ev2gym.models.grid_utility.grid_tensor import GridTensor
    import ev2gym
    data = os.path.join(os.path.dirname(ev2gym.__file__), "data", "network_data")
    bus_csv, branch_csv = os.path.join(data, bus_csv), os.path.join(data, branch_csv)
    net = GridTensor(bus_csv, branch_csv)
    n = n_bus - 1
    assert net.nb == n_bus
    rng = np.random.default_rng(seed)
    nominal = net.p_values[1:]
    by_count, refused = {}, 0
    # low scales first: the short counts are the rare ones
    for scale in np.concatenate([[0.0], rng.uniform(0.3, 3.0, 400)]):
        P_load = np.round(nominal * np.clip(scale * rng.uniform(0.8, 1.2, n), 0.3 if scale else 0.0, 3.0), 1)
        Q = np.round(P_load * net.pf, 1).reshape(1, -1)
        P = (P_load + (np.round(rng.uniform(-22.0, 22.0, n), 3) if scale else 0.0)).reshape(1, -1)
        sol = net.run_pf(active_power=P.copy(), reactive_power=Q.copy())
        it = int(sol["iterations"])
        if not sol["convergence"]:
            refused += 1
            print("  refused: the reference's solver did not converge")
            continue
        res = (residual(net, P, Q, it - 1), residual(net, P, Q, it))
        if near(res[0]) or near(res[1]):
            refused += 1
            print(f"  refused: residuals {res} within {GUARD:g} of the tolerance")
            continue
        assert res[1] < TOL <= res[0], (it, res)   # the count the reference reported is the one its residuals give
        by_count.setdefault(it, []).append((P[0], Q[0], sol["v"][0].copy(), it, res))
    counts = sorted(by_count)
    print(f"{n_bus} buses: iteration counts {dict((c, len(by_count[c])) for c in counts)}, {refused} refused")
    cases, k = [], 0
    while len(cases) < N_CASES:   # round robin over the counts: neighbours differ
        c = counts[k % len(counts)]
        k += 1
        if by_count[c]:
            cases.append(by_count[c].pop(0))
        elif not any(by_count.values()):
            raise SystemExit("not enough cases passed the iteration-count guard")
    P, Q, v = (np.array([c[i] for c in cases]) for i in range(3))
    iters, res = np.array([c[3] for c in cases], np.int32), np.array([c[4] for c in cases])
    vm = np.concatenate([np.ones((len(cases), 1)), np.abs(v)], axis=1)

    # PowerGrid.reset / step on caller-supplied profiles
    T = 3
    load = np.round(net.p_values * rng.uniform(0.3, 1.2, (T + 1, n_bus)), 1)
    pv = np.round(net.p_values * rng.uniform(0.0, 0.5, (T + 1, n_bus)), 1)
    ev = np.round(rng.uniform(-22.0, 22.0, (T, n)), 3)
    g = PowerGrid.__new__(PowerGrid)
    g.net, g.node_num = net, n_bus
    a, r = g.reset(datetime.datetime(2022, 1, 17, 5, 0), load.copy(), pv.copy())   # (reset subtracts the PV from its argument's row 0 in place)
    traj_p, traj_q, traj_vm = [a.copy()[0]], [r.copy()[0]], []
    for t in range(T):
        a, r, m = g.step(ev[t].copy())
        traj_p.append(a.copy()[0]); traj_q.append(r.copy()[0]); traj_vm.append(np.asarray(m).copy())
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"grid_{n_bus}.npz"), K=net._K_, L=np.asarray(net._L_).reshape(-1), pf=net.pf, s_base=float(net.s_base),
                        tolerance=TOL, P=P, Q=Q, v=v, vm=vm, iters=iters, res=res, traj_load=load, traj_pv=pv, traj_ev=ev,
                        traj_p=np.array(traj_p), traj_q=np.array(traj_q), traj_vm=np.array(traj_vm))
    for f in (bus_csv, branch_csv):
        shutil.copyfile(f, os.path.join(OUT, os.path.basename(f)))
        os.chmod(os.path.join(OUT, os.path.basename(f)), 0o644)
    print(f"  wrote grid_{n_bus}.npz: {len(cases)} cases, counts {iters.tolist()}")


if __name__ == "__main__":
    from oracle.ref_import import import_reference
    import_reference()
    import warnings
    warnings.simplefilter("ignore")
    for net in NETWORKS:
        capture(*net)
