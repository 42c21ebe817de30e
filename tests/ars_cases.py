"""Cases shared by tests/test_ars_cpu.py, tests/test_ars_gpu.py and tests/test_ars_range_gpu.py: update cases with distinct scores, sb3_contrib's
update lines restated in torch float64, the crafted return vectors, and random policies of every network the tests run.

For the range module: EDGE_NETS (the networks at the edges of what plan_ars accepts) with edge_case's pinned draws; MANY / many_case (8192
candidates of one row, 514 of 33 rows); LARGE_UPDATES / large_update / large_returns (n_delta 255 .. 4096 with distinct, tied, NaN and infinite
returns).  The candidates and directions of these cases come from the host twin of the perturb launch, which the GPU modules hold the device to
bit for bit, so what the CPU module pins on the float64 reference is pinned for the very weights the device runs."""
import numpy as np

# (n_delta, n_top) of the update cases: n_top = n_delta, n_top < n_delta, n_top = 1, n_delta = 1
UPDATE_CASES = [(8, 8), (8, 3), (8, 1), (1, 1)]
# network tag -> (kind, D, h1, h2, P)
NETS = {
    "pst-64-64": ("MlpPolicy", 63, 64, 64, 20), "ppl-64-64": ("MlpPolicy", 162, 64, 64, 50), "pst-33-17": ("MlpPolicy", 63, 33, 17, 20),
    "ppl-33-17": ("MlpPolicy", 162, 33, 17, 50), "pst-256-256": ("MlpPolicy", 63, 256, 256, 20), "ppl-256-256": ("MlpPolicy", 162, 256, 256, 50),
    "pst-linear": ("LinearPolicy", 63, 0, 0, 20), "ppl-linear": ("LinearPolicy", 162, 0, 0, 50),
}
# the networks at the edges of what plan_ars accepts (D 1..192, hidden widths 1..256, P 1..64; k1 = D to 8, n = widths and P to 32):
#   limits      every maximum, no padded port              tile        no padding in any dimension (k1 == D, n == h, n3 == P)
#   tile+1      k1 16, n1 = n2 = n3 = 64: every guard acts  eighth      P 57: write-out lane 0 of the eight takes ports 0, 8, ..., 56
#   tiny        one input, one port, widths 5 and 2        lin-*       the linear policy at the limits, one past the tile, and 1 -> 1
EDGE_NETS = {
    "limits": ("MlpPolicy", 192, 256, 256, 64), "tile": ("MlpPolicy", 8, 32, 32, 32), "tile+1": ("MlpPolicy", 9, 33, 33, 33),
    "eighth": ("MlpPolicy", 63, 64, 64, 57), "tiny": ("MlpPolicy", 1, 5, 2, 1),
    "lin-limits": ("LinearPolicy", 192, 0, 0, 64), "lin-tile+1": ("LinearPolicy", 9, 0, 0, 33), "lin-tiny": ("LinearPolicy", 1, 0, 0, 1),
}
EDGE_C, EDGE_R, EDGE_STD, EDGE_SEED = (2, 6), (1, 32, 33), 0.1, 5   # candidates, rows per candidate, delta_std and the objects' seed of the edge cases
# the population launches with many candidates: name -> (tag, n_delta, R)
MANY = {"8192x1": ("pst-linear", 4096, 1), "514x33": ("pst-33-17", 257, 33)}
# (n_delta, n_top) of the large updates: around the rank kernel's 256 threads, n_top = n_delta, n_top = 1, n_top < n_delta on either side of 256, the plan's limit
LARGE_UPDATES = [(255, 255), (256, 100), (257, 257), (257, 1), (1000, 256), (4096, 4096), (4096, 257)]
LARGE_KINDS = ("distinct", "ties", "nan", "inf")
LARGE_INF_AT = 300   # the candidate that holds +inf in the "inf" returns: above the first 256


def update_case(n_delta, n_top, n_params=57, seed=0):
    """theta, delta, returns [2 n_delta] with pairwise distinct scores max(r+, r-)"""
    rng = np.random.default_rng(1000 * n_delta + 10 * n_top + seed)
    theta = rng.normal(0.0, 0.3, n_params).astype(np.float32)
    delta = rng.normal(size=(n_delta, n_params)).astype(np.float32)
    returns = rng.normal(-50.0, 20.0, 2 * n_delta)
    return dict(theta=theta, delta=delta, returns=returns, n_delta=n_delta, n_top=n_top, lr=0.02)


def scores(returns):
    n = len(returns) // 2
    return np.maximum(returns[:n], returns[n:])


def torch_update(case):
    """sb3_contrib's ARS._do_one_update lines, float64: (new theta, sigma_R, step, top_idx)"""
    import torch as th
    theta, delta = th.from_numpy(case["theta"].astype(np.float64)), th.from_numpy(case["delta"].astype(np.float64))
    r = th.from_numpy(np.asarray(case["returns"], np.float64))
    n_delta, n_top = case["n_delta"], case["n_top"]
    plus_returns, minus_returns = r[:n_delta], r[n_delta:]
    top_returns, _ = th.max(th.vstack((plus_returns, minus_returns)), dim=0)
    top_idx = th.argsort(top_returns, descending=True)[:n_top]
    plus_returns, minus_returns, deltas = plus_returns[top_idx], minus_returns[top_idx], delta[top_idx]
    return_std = th.cat([plus_returns, minus_returns]).std()
    step_size = case["lr"] / (n_top * return_std + 1e-6)
    new = theta + step_size * ((plus_returns - minus_returns) @ deltas)
    return new.numpy(), float(return_std), float(step_size), top_idx.numpy()


def crafted_returns(n_delta=4):
    """name -> returns [2 n_delta]: ties (equal scores), all equal, a NaN, an infinity"""
    base = np.array([3.0, -1.0, 7.5, 2.0, 0.5, 4.0, 4.0, 2.5][:2 * n_delta], np.float64)
    ties = np.array([5.0, 1.0, 5.0, 0.0, 2.0, 5.0, 3.0, 5.0][:2 * n_delta], np.float64)   # every score is 5
    nan, inf = base.copy(), base.copy()
    nan[5], inf[2] = np.nan, -np.inf
    return {"plain": base, "ties": ties, "equal": np.full(2 * n_delta, -12.5), "nan": nan, "inf": inf}


def net_of(tag):
    """(kind, D, h1, h2, P) of a NETS or EDGE_NETS tag"""
    return NETS[tag] if tag in NETS else EDGE_NETS[tag]


def n_params_of(tag):
    from ev2gym_amd import _abi
    return sum(int(np.prod(s)) for s in _abi.ars_param_shapes(*net_of(tag)))


def random_theta(tag, seed=0, scale=1.0):
    """A policy's parameter vector with torch.nn.Linear-style uniform(-1/sqrt(in), 1/sqrt(in)) arrays (times `scale`), float32"""
    from ev2gym_amd import _abi
    kind, D, h1, h2, P = net_of(tag)
    rng = np.random.default_rng(seed + 17 * D + P)
    parts = []
    fan = 1
    for s in _abi.ars_param_shapes(kind, D, h1, h2, P):
        if len(s) == 2:
            fan = s[1]
        k = scale / np.sqrt(fan)
        parts.append(rng.uniform(-k, k, s).astype(np.float32).ravel())
    return np.concatenate(parts)


# ---- the edge cases of the population forward ----
def saturated_ports(P):
    """port -> the shift of its output bias in the saturated case: +12, -12, +12, ... on every second port"""
    return {p: (12.0 if (p // 2) % 2 == 0 else -12.0) for p in range(0, P, 2)}


def _pre_tanh(x, w):
    """float64 pre-activations of the MLP policy's tanh [n, P]"""
    w = [np.asarray(a, np.float64) for a in w]
    h = np.maximum(np.maximum(np.asarray(x, np.float64) @ w[0].T + w[1], 0.0) @ w[2].T + w[3], 0.0)
    return h @ w[4].T + w[5]


def _draw_edge(tag, lo, seed, saturate):
    from ev2gym_amd.ars import ars_forward_numpy, split_theta
    from ev2gym_amd.engine import host_ars_perturb
    kind, D, h1, h2, P = net_of(tag)
    theta = random_theta(tag, seed)
    sat = saturated_ports(P) if saturate else {}
    if sat:
        b3 = split_theta(theta, kind, D, h1, h2, P)[5]   # (a view of theta)
        for p, shift in sat.items():
            b3[p] += np.float32(shift)
    rows = np.random.default_rng(seed + 7 * D + P + int(lo)).normal(size=(max(EDGE_R), D)).astype(np.float32)
    case = dict(tag=tag, lo=lo, seed=seed, theta=theta, rows=rows, sat=sat, cands={}, refs={}, figures={}, misses=[])
    free = np.array([p not in sat for p in range(P)])
    for C in EDGE_C:
        _, cand = host_ars_perturb(theta, C // 2, EDGE_STD, EDGE_SEED, 0)   # the candidates the device's first perturb writes, bit for bit
        case["cands"][C] = cand
        arrays = [split_theta(cand[c], kind, D, h1, h2, P) for c in range(C)]
        full = np.stack([ars_forward_numpy(rows, arrays[c], kind, lo) for c in range(C)])
        fig = case["figures"][C] = {}
        for R in EDGE_R:
            case["refs"][C, R] = full[:, :R]
            apart = min(float(np.abs(full[c, :R] - full[c2, :R]).max()) for c in range(C) for c2 in range(c))
            fig[f"apart R {R}"] = apart
            if not apart > 1e-3:
                case["misses"].append(f"C {C} R {R}: two candidates' actions are only {apart:.3e} apart")
        if kind == "MlpPolicy":
            v = np.stack([_pre_tanh(rows, arrays[c]) for c in range(C)])
            fig["|v| > 9"] = share = float((np.abs(v[..., free]) > 9.0).mean())
            fig["median |v|"] = float(np.median(np.abs(v[..., free])))
            if not share < 0.10:
                case["misses"].append(f"C {C}: {share:.3f} of the tanh pre-activations exceed 9")
            if sat:
                fig["least saturated |v|"] = least = float(np.abs(v[..., ~free]).min())
                signs_ok = all((np.sign(v[..., p]) == np.sign(s)).all() for p, s in sat.items())
                if not (least >= 10.0 and signs_ok):
                    case["misses"].append(f"C {C}: a saturated port's pre-activation is only {least:.3f}, or of the other sign")
        elif full.size >= 256:
            fig["at lo"], fig["at 1"] = at_lo, at_1 = float((full == lo).mean()), float((full == 1.0).mean())
            fig["inside"] = inside = float(((full > lo) & (full < 1.0)).mean())
            if not (at_1 >= 0.02 and at_lo >= (0.02 if lo == -1.0 else 0.30) and inside >= 0.15):
                case["misses"].append(f"C {C}: shares at lo {at_lo:.3f}, at 1 {at_1:.3f}, inside {inside:.3f}")
    return case


def edge_case(tag, lo, saturate=False):
    """An EDGE_NETS network with theta at torch.nn.Linear's scale, 33 standard normal rows and, for C in EDGE_C, the candidates of the first
    perturb under (EDGE_SEED, EDGE_STD), with the float64 actions refs[C, R] [C, R, P] of every row under its own candidate.  Pinned on that
    reference alone (case["misses"] lists what a draw misses; the CPU module asserts it is empty):
      * at every C and R the candidates' actions are pairwise more than 1e-3 apart;
      * MlpPolicy: fewer than 10 % of the tanh pre-activations exceed 9 in magnitude (on the unshifted ports);
      * LinearPolicy with at least 256 output elements: at least 2 % of them at each bound (lo = 0: 2 % at 1 and 30 % at lo), 15 % strictly inside;
      * saturate (output bias moved by +-12 on every second port, saturated_ports): |pre-activation| >= 10 with the shift's sign on those
        ports, so the float64 action is within 5e-9 of the bound and rounds to exactly 1 or lo in float32.
    The first of ten fixed seeds (0, 1000, ...) that misses nothing is taken (tests/td3_cases.make_case's idiom; one row of a 1 -> 1 linear
    policy is clipped to the same bound for two candidates about every other seed); case["seeds_skipped"] counts the ones passed over."""
    for i in range(10):
        case = _draw_edge(tag, lo, 1000 * i, saturate)
        case["seeds_skipped"] = i
        if not case["misses"]:
            break
    return case


_CACHE = {}


def many_case(name):
    """A population launch with many candidates (MANY): theta, the rows x [C R, D], the first perturb's candidates under (EDGE_SEED, EDGE_STD)
    from the host twin, and the float64 actions ref [C, R, P] of every row under its own candidate, lo = -1.  Built once."""
    if name not in _CACHE:
        from ev2gym_amd.ars import ars_forward_numpy, split_theta
        from ev2gym_amd.engine import host_ars_perturb
        tag, n_delta, R = MANY[name]
        kind, D, h1, h2, P = net_of(tag)
        C = 2 * n_delta
        theta = random_theta(tag)
        x = np.random.default_rng(n_delta + R).normal(size=(C * R, D)).astype(np.float32)
        _, cand = host_ars_perturb(theta, n_delta, EDGE_STD, EDGE_SEED, 0)
        ref = np.stack([ars_forward_numpy(x[c * R:(c + 1) * R], split_theta(cand[c], kind, D, h1, h2, P), kind, -1.0) for c in range(C)])
        _CACHE[name] = dict(tag=tag, n_delta=n_delta, R=R, C=C, theta=theta, x=x, cand=cand, ref=ref)
    return _CACHE[name]


# ---- the large updates ----
def large_returns(n_delta, n_top, kind):
    """returns [2 n_delta] of a large update:
      distinct  N(-50, 20), the scores pairwise distinct (asserted by the CPU module);
      ties      integer-valued, drawn from eight values, so that equal scores stand on both sides of the n_top cut; past 256 directions,
                direction 256 is given direction 0's two returns, so that k and k + 256 tie (one thread of the rank kernel ranks both);
      nan       `distinct` with a NaN at the last candidate, 2 n_delta - 1;     inf: `distinct` with +inf at candidate LARGE_INF_AT."""
    rng = np.random.default_rng(100000 * n_delta + n_top)
    r = rng.normal(-50.0, 20.0, 2 * n_delta)
    if kind == "ties":
        r = rng.integers(-3, 5, 2 * n_delta).astype(np.float64)
        if n_delta > 256:
            r[256], r[n_delta + 256] = r[0], r[n_delta]
    elif kind == "nan":
        r[2 * n_delta - 1] = np.nan
    elif kind == "inf":
        r[LARGE_INF_AT] = np.inf
    elif kind != "distinct":
        raise KeyError(kind)
    return r


def large_update(n_delta):
    """theta of pst-linear (1260 parameters) and the directions [n_delta, 1260] of its first perturb under EDGE_SEED, from the host twin; lr 0.02"""
    key = ("update", n_delta)
    if key not in _CACHE:
        from ev2gym_amd.engine import host_ars_perturb
        theta = random_theta("pst-linear")
        delta, _ = host_ars_perturb(theta, n_delta, 0.05, EDGE_SEED, 0)
        for k in [k for k in _CACHE if k[0] == "update"]:   # (one n_delta's directions at a time: 20 MB at 4096)
            del _CACHE[k]
        _CACHE[key] = dict(theta=theta, delta=delta, lr=0.02, delta_std=0.05)
    return _CACHE[key]


def stable_ranks(returns):
    """direction k's rank under "score descending, ties to the lower index", from numpy's stable argsort"""
    s = scores(returns)
    rank = np.empty(len(s), np.int64)
    rank[np.argsort(-s, kind="stable")] = np.arange(len(s))
    return rank
