"""What tests/test_td3_cpu.py and tests/test_td3_gpu.py share: the case builder of one TD3 / DDPG batch (rows redrawn away from ReLU's kinks),
the torch restatement of SB3's TD3.train() in either precision (autograd, torch.optim.Adam(eps=1e-8), polyak_update's mul_ / add_), and the
comparison under the project's tolerance idiom (tests/test_ppo_gpu.py's docstring).  A plain module."""
import numpy as np

from tests.test_ppo_cpu import _record, grad_tol, value_tol

NETS = {"400-300": (400, 300), "64-64": (64, 64), "33-17": (33, 17)}
KINK = 1e-5   # no float64 pre-activation of a backpropagated ReLU layer is nearer to 0 than this
# The plan's limits and the product kernel's tile edges (csrc/ev2g_td3_host.h: D <= 192, P <= 64, hidden widths 1 .. 400; csrc/ev2g_td3.h: 16 x 16
# tiles, column sums over 16-column blocks): tag -> (D, h1, h2, P).  A table of its own: the _grad_cases() of the GPU modules cycle over NETS.
#   limits   every plan maximum: 25 tiles per hidden layer, none ragged; the bound policy runs ev2g_mlp3_any (h2 > 304)
#   tile     exactly one tile in every dimension: one trip of the k loop with kn = 16
#   tile+1   every dimension ragged by one: the kn tail of 1, and the m < M / n < N / ka < K guards all act
#   tiny     D 1, P 1, a critic input of 2 columns: layers narrower than a tile
EDGE_NETS = {"limits": (192, 400, 400, 64), "tile": (16, 16, 16, 16), "tile+1": (17, 17, 33, 17), "tiny": (1, 5, 2, 1)}
SATURATED = 12.0   # |output bias shift| of a saturated port: float32 tanh is exactly +-1 above about 9.01, in torch and on the device alike


# (tag, n_critics, lo, sigma, B): B in {1, 33, 1023, 1024} at limits -- 1024 is the one size at which the z strides (from B) and the workspace's
# layout (for 1024 rows) coincide, 1023 leaves the last row tile and block_sum's last trip ragged -- and {33, 1024} elsewhere; n_critics, lo and
# sigma are spread so that each value meets each network, and both large batches at limits run two critics (the z dimension).
EDGE_GRAD_CASES = [("limits", 1, 0.0, 0.2, 1), ("limits", 1, -1.0, 0.0, 33), ("limits", 2, -1.0, 0.0, 1023), ("limits", 2, 0.0, 0.2, 1024),
                   ("tile", 2, -1.0, 0.2, 33), ("tile", 1, 0.0, 0.0, 1024), ("tile+1", 1, -1.0, 0.2, 33), ("tile+1", 2, 0.0, 0.0, 1024),
                   ("tiny", 2, 0.0, 0.0, 33), ("tiny", 1, -1.0, 0.2, 1024)]
# (net, (D, P), n_critics, lo, sigma, B) with a saturated actor
# (the third has no noise: half of its a' elements are exactly +-1 by construction, whatever the draws)
SATURATED_GRAD_CASES = [("64-64", (63, 20), 2, -1.0, 0.2, 100), ("limits", (192, 64), 2, 0.0, 0.2, 33), ("64-64", (63, 20), 1, 0.0, 0.0, 100)]
# the networks of the refresh test off the handles' shapes: (tag, (D, h1, h2, P), precision, the kernel the plan gives).  The second shape is the
# nearest one to 170-410-300-50 that plan_td3 accepts (h1 <= 400; the GPU test shows the refusal): 16-column tile counts 11 / 26 / 20 all the same.
REFRESH_EDGE_CASES = [("limits", EDGE_NETS["limits"], "bf16", "ev2g_mlp3_any"), ("limits", EDGE_NETS["limits"], "fp32", "ev2g_mlp3_f32"),
                      ("fixed", (170, 400, 310, 50), "bf16", "ev2g_mlp3_fixed<11,26,20>")]


def edge_grad_case(tag, n_critics, lo, sigma, B):
    return edge_case(tag, n_critics, B, lo, sigma, seed=7 + B, first_draw=1000)


def saturated_grad_case(net, dp, n_critics, lo, sigma, B):
    return make_case(*dp, net, n_critics, B, lo, sigma, seed=7 + B, first_draw=1000, saturate=True, live=True)


def _hidden(net):
    return NETS[net] if net in NETS else EDGE_NETS[net][1:3] if net in EDGE_NETS else tuple(net)


def edge_case(tag, *args, **kw):
    """make_case on a row of EDGE_NETS, with the live-gradient condition."""
    D, _, _, P = EDGE_NETS[tag]
    return make_case(D, P, tag, *args, live=True, **kw)


def saturated_ports(P):
    """every second port, and the sign of its shift: +, -, +, ..."""
    ports = np.arange(0, P, 2)
    return ports, np.where(np.arange(ports.size) % 2 == 0, 1.0, -1.0)


def nonzero_grads(ref):
    """every float64 reference gradient array of a case has a non-zero element (a dead ReLU in a narrow network makes whole arrays exactly 0, and
    zero against zero proves nothing)"""
    return all(np.any(g) for c in ref["critic_grads"] for g in c) and all(np.any(g) for g in ref["actor_grads"])


def _min_preact(case, rows):
    """Per row: the smallest |pre-activation| over every ReLU layer that is backpropagated through (float64)."""
    from ev2gym_amd.td3 import _forward, _f64, scale_action
    s = case["obs"][rows].astype(np.float64)
    a = scale_action(case["actions"][rows].astype(np.float64), case["lo"])
    fa = _forward(_f64(case["actor"]), s, True)
    fs = [fa] + [_forward(_f64(c), np.concatenate([s, a], 1), False) for c in case["critics"]]
    fs.append(_forward(_f64(case["critics"][0]), np.concatenate([s, fa.out], 1), False))
    return np.min([np.minimum(np.abs(f.z1).min(1), np.abs(f.z2).min(1)) for f in fs], axis=0)


def make_case(D, P, net="400-300", n_critics=2, B=37, lo=-1.0, sigma=0.2, seed=7, noise_seed=11, first_draw=0, saturate=False, live=False):
    """_draw_case(seed), asserting that fewer than a quarter of the rows needed a redraw.  With ONE row a quarter means none, which a given seed
    misses about one time in twenty: only then the first of ten fixed seeds (seed, seed + 1000, ...) that needs no redraw is taken, as the ReLU
    cases of tests/test_ppo_cpu.py take the first of ten seeds that fits.  A larger batch gets no second seed, so a redraw rate that drifted
    upwards fails here.  case["seeds_skipped"] says how many seeds were passed over; the tests print it next to the redraw count.

    live (the EDGE_NETS and the saturated cases): every float64 reference gradient array must also have a non-zero element (nonzero_grads), and a
    seed that misses that or the cap is passed over at any B, again among the ten fixed seeds.  The float64 reference is kept as case["ref64"].
    saturate: see _draw_case; at least a quarter of the a' elements must be exactly +-1.  With noise that is the EXPECTATION -- half the ports
    times the half of the draws that point outwards -- and it depends on (noise_seed, first_draw) alone, not on the seed: the cases' draws give
    0.26, and other draws can miss it.  Without noise the share is a half by construction, and that is asserted."""
    import torch
    for i in range(10 if (B == 1 or live) else 1):
        case = _draw_case(D, P, net, n_critics, B, lo, sigma, seed + 1000 * i, noise_seed, first_draw, saturate)
        case["seeds_skipped"] = i
        ok = case["redrawn"] < B / 4.0
        if live and ok:
            case["ref64"] = torch_grads(case, torch.float64)
            ok = nonzero_grads(case["ref64"])
        if ok:
            break
    assert case["redrawn"] < B / 4.0, f"{case['redrawn']} of {B} rows needed a redraw"
    if live:
        assert nonzero_grads(case["ref64"]), "a reference gradient array is all zeros (dead ReLU)"
    if saturate:
        assert case["share_at_1"] >= (0.25 if sigma > 0.0 else 0.5), f"only {case['share_at_1']:.3f} of the a' elements are exactly +-1"
    return case


def _draw_case(D, P, net, n_critics, B, lo, sigma, seed, noise_seed, first_draw, saturate=False):
    """One batch and the networks of a learner: torch-style initial weights, observations in [0, 1], stored actions in [lo, 1], rewards of both
    signs, `done` mixed, the smoothing noise's standard normals from the host twin.  Rows with a pre-activation inside KINK are redrawn.
    saturate: the actor's output bias of every second port is moved by +12, -12, +12, ... BEFORE the redraws, so that |pre-tanh| >= 10 in
    float64 on those ports for every row of obs and next_obs (asserted): tanh_back's 1 - t^2 at t = +-1 and the clamp a' in [-1, 1] are reached.
    The band 3 .. 9, where the result depends on each tanhf's last bits, is left out on purpose.  case["share_at_1"]: the share of float32 a'
    elements that are exactly +-1."""
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import host_normal
    from ev2gym_amd.td3 import init_critic_weights
    h1, h2 = _hidden(net)
    rng = np.random.default_rng(seed)
    case = dict(D=D, P=P, h=(h1, h2), n_critics=n_critics, B=B, lo=float(lo), sigma=float(sigma), clip=0.5, gamma=0.99, noise_seed=noise_seed,
                first_draw=first_draw, actor=init_mlp_weights(D, P, seed, h1, h2),
                critics=[init_critic_weights(D, P, seed + 1 + j, h1, h2) for j in range(n_critics)])
    if saturate:
        ports, sign = saturated_ports(P)
        case["actor"][5][ports] += (SATURATED * sign).astype(np.float32)
    case["obs"] = rng.uniform(0.0, 1.0, (B, D)).astype(np.float32)
    case["actions"] = rng.uniform(lo, 1.0, (B, P)).astype(np.float32)
    case["reward"] = rng.normal(0.0, 1.0, B).astype(np.float32)
    case["next_obs"] = rng.uniform(0.0, 1.0, (B, D)).astype(np.float32)
    case["done"] = (rng.uniform(size=B) < 0.3).astype(np.uint8)
    if B > 1:
        case["done"][:2] = (0, 1)
    case["normals"] = host_normal(B * P, noise_seed, first_draw).reshape(B, P) if sigma > 0.0 else None
    redrawn = np.zeros(B, bool)
    for _ in range(50):
        bad = np.nonzero(_min_preact(case, np.arange(B)) < KINK)[0]
        if bad.size == 0:
            break
        redrawn[bad] = True
        case["obs"][bad] = rng.uniform(0.0, 1.0, (bad.size, D)).astype(np.float32)
        case["actions"][bad] = rng.uniform(lo, 1.0, (bad.size, P)).astype(np.float32)
    assert _min_preact(case, np.arange(B)).min() >= KINK, "a row still sits on a ReLU kink"
    case["redrawn"] = int(redrawn.sum())
    if saturate:
        from ev2gym_amd.engine import host_td3_target
        from ev2gym_amd.td3 import _f64, _forward
        ports, _ = saturated_ports(P)
        w = _f64(case["actor"])
        for x in (case["obs"], case["next_obs"]):
            f = _forward(w, x.astype(np.float64), True)
            z3 = f.h2 @ w[4].T + w[5]
            assert np.abs(z3[:, ports]).min() >= 10.0, "a saturated port's pre-tanh is inside 10"
        a_next, _ = host_td3_target(np.tanh(z3).astype(np.float32), None, None, None, sigma, case["clip"], case["gamma"], noise_seed, first_draw)
        case["share_at_1"] = float((np.abs(a_next) == 1.0).mean())
    return case


def torch_nets(case, dtype):
    import torch
    mk = lambda ws: [torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(True) for a in ws]  # noqa: E731
    return mk(case["actor"]), [mk(c) for c in case["critics"]]


def _mlp(w, x, tanh):
    import torch
    F = torch.nn.functional
    z = F.linear(torch.relu(F.linear(torch.relu(F.linear(x, w[0], w[1])), w[2], w[3])), w[4], w[5])
    return torch.tanh(z) if tanh else z


def _batch(case, dtype, rows=None):
    import torch
    sl = slice(None) if rows is None else rows
    t = lambda a: torch.tensor(np.asarray(a)[sl], dtype=dtype)  # noqa: E731
    s, a, r, s2, d = t(case["obs"]), t(case["actions"]), t(case["reward"]), t(case["next_obs"]), t(case["done"])
    if case["lo"] == 0.0:
        a = 2.0 * a - 1.0
    return s, a, r, s2, d


def torch_critic_loss(case, dtype, actor_t, critics, critics_t, batch, normals):
    """(critic_loss, y) as SB3 writes them."""
    import torch
    s, a, r, s2, d = batch
    with torch.no_grad():
        at = _mlp(actor_t, s2, True)
        if normals is not None and case["sigma"] > 0.0:
            at = at + (torch.tensor(normals, dtype=dtype) * case["sigma"]).clamp(-case["clip"], case["clip"])
        a2 = at.clamp(-1.0, 1.0)
        tq = torch.cat([_mlp(c, torch.cat([s2, a2], 1), False) for c in critics_t], 1).min(1).values
        y = r + (1.0 - d) * case["gamma"] * tq
    xa = torch.cat([s, a], 1)
    return sum(torch.nn.functional.mse_loss(_mlp(c, xa, False)[:, 0], y) for c in critics), y


def torch_grads(case, dtype):
    """One staged step (critic gradient, then the actor's through the UNCHANGED critic_0) by autograd: dict of y, critic_loss, actor_loss,
    critic_grads (a list of six per critic), actor_grads as float64 numpy."""
    import torch
    actor, critics = torch_nets(case, dtype)
    batch = _batch(case, dtype)
    closs, y = torch_critic_loss(case, dtype, [a.detach() for a in actor], critics, [[a.detach() for a in c] for c in critics], batch, case["normals"])
    cg = torch.autograd.grad(closs, [a for c in critics for a in c])
    s = batch[0]
    aloss = -_mlp(critics[0], torch.cat([s, _mlp(actor, s, True)], 1), False).mean()
    ag = torch.autograd.grad(aloss, actor)
    n = lambda x: x.detach().double().numpy()  # noqa: E731
    return dict(y=n(y), critic_loss=float(closs.detach().double()), actor_loss=float(aloss.detach().double()),
                critic_grads=[[n(g) for g in cg[6 * j:6 * j + 6]] for j in range(case["n_critics"])], actor_grads=[n(g) for g in ag])


def torch_loop(case, batches, dtype, policy_delay=2, lr=1e-3, tau=0.005):
    """SB3's TD3.train() over `batches` (a list of (row indices, normals or None)): per step a dict of critic_loss, actor_loss (None without
    an actor step), and float64 copies of the masters and targets (actor, critics, actor_target, critics_target) after the step."""
    import torch
    actor, critics = torch_nets(case, dtype)
    actor_t = [a.detach().clone() for a in actor]
    critics_t = [[a.detach().clone() for a in c] for c in critics]
    opt_a = torch.optim.Adam(actor, lr=lr, eps=1e-8)
    opt_c = torch.optim.Adam([a for c in critics for a in c], lr=lr, eps=1e-8)
    out = []
    n = lambda ws: [a.detach().double().numpy().copy() for a in ws]  # noqa: E731
    for k, (rows, normals) in enumerate(batches, 1):
        batch = _batch(case, dtype, rows)
        closs, _ = torch_critic_loss(case, dtype, actor_t, critics, critics_t, batch, normals)
        opt_c.zero_grad(); closs.backward(); opt_c.step()
        aloss = None
        if k % policy_delay == 0:
            s = batch[0]
            aloss = -_mlp(critics[0], torch.cat([s, _mlp(actor, s, True)], 1), False).mean()
            opt_a.zero_grad(); aloss.backward(); opt_a.step()
            with torch.no_grad():
                for tgt, src in zip([a for c in critics_t for a in c] + actor_t, [a for c in critics for a in c] + actor):
                    tgt.mul_(1.0 - tau)
                    torch.add(tgt, src, alpha=tau, out=tgt)
            aloss = float(aloss.detach().double())
        out.append(dict(critic_loss=float(closs.detach().double()), actor_loss=aloss, actor=n(actor), critics=[n(c) for c in critics],
                        actor_target=n(actor_t), critics_target=[n(c) for c in critics_t]))
    return out


def check_arrays(tag, got, ref, ref32, values=False, plain32=None):
    """Lists of arrays under the idiom: prints every d32 and deviation, then asserts.  plain32: a second float32 computation whose d32 is
    printed next to the one that sets the tolerance (the saturated SAC cases, tests/sac_cases.torch_actor's `mixed`)."""
    fails = []
    for i, (g, r, r32) in enumerate(zip(got, ref, ref32)):
        g, r, r32 = np.asarray(g, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1), np.asarray(r32, np.float64).reshape(-1)
        d32 = float(np.abs(r32 - r).max())
        tol = value_tol(r, d32) if values else grad_tol(r, d32)
        dev = np.abs(g - r)
        also = "" if plain32 is None else f" (plain float32 d32 {float(np.abs(np.asarray(plain32[i], np.float64).reshape(-1) - r).max()):.3e})"
        _record(f"{tag}[{i}] d32 {d32:.3e}{also} device {float(dev.max()):.3e} tol {float(np.max(tol)):.3e} scale {float(np.abs(r).max()):.3e}")
        if not np.all(dev <= tol):
            fails.append((i, float(dev.max()), float(np.max(tol))))
    assert not fails, (tag, fails)


# ---- the replay ring and its sampler (tests/test_td3_gpu.py and tests/test_sac_gpu.py) ----
def snapshot(col, block):
    """host copies of a ring block: (obs [T + 1, E, D], actions, reward, done)"""
    return [a.to_host() for a in (col.obs[block], col.actions[block], col.reward[block], col.done[block])]


def gather(blocks, idx, T):
    """The rows of host copies of the listed blocks at idx [B, 3] (entry of the list, t, e)."""
    bi, t, e = idx[:, 0], idx[:, 1], idx[:, 2]
    pick = lambda k, tt: np.stack([blocks[b][k][x, y] for b, x, y in zip(bi, tt, e)])  # noqa: E731
    return pick(0, t), pick(1, t), pick(2, t).astype(np.float32), pick(0, t + 1), pick(3, t)


def check_sample(col, ring, host, B, seed, counters):
    """ev2g_replay_sample on the device list `ring` for every counter: the indices are the host twin's, every row is the gather from `host` (the
    listed blocks' host copies) bit for bit, s' of a last step is the block's row T.  Returns the indices."""
    from ev2gym_amd.engine import host_replay_indices
    from tests.test_onpolicy_gpu import _bits
    eng, T, E, D, P = col.eng, col.T, col.E, col.D, col.P
    out = [eng.empty((B, D), np.float32), eng.empty((B, P), np.float32), eng.empty((B,), np.float32), eng.empty((B, D), np.float32), eng.empty((B,), np.uint8)]
    index = eng.empty((B, 3), np.int32)
    seen = []
    try:
        for counter in counters:
            eng.replay_sample(ring, T, E, D, P, B, seed, counter, *out, index)
            idx = index.to_host()
            assert np.array_equal(idx, host_replay_indices(B, len(ring), T, E, seed, counter))
            assert idx[:, 0].min() == 0 and idx[:, 0].max() == len(ring) - 1 and idx[:, 1].max() == T - 1 and idx[:, 1].min() == 0
            got = [o.to_host() for o in out]
            for a, b in zip(got, gather(host, idx, T)):
                assert np.array_equal(_bits(a), _bits(b))
            last = idx[:, 1] == T - 1
            assert last.any()
            for r in np.nonzero(last)[0]:
                assert np.array_equal(got[3][r], host[idx[r, 0]][0][T, idx[r, 2]])
            seen.append(idx)
    finally:
        for b in out + [index]:
            b.free()
    return seen


def check_ring_wrap(col, learner, B=256):
    """Four episodes into a ring of capacity 3: the head wraps, the complete blocks are [0, 2] -- not contiguous -- with episode 4 in block 0 over
    episode 1 and episode 3 in block 2; block 1 holds the stale episode 2 under the next reset row and is never drawn.  The sampler, on exactly the
    list train() builds, gathers from the snapshots of episodes 4 and 3 (the snapshots are taken as each block fills)."""
    assert col.cap == 3
    snaps = []
    for ep in range(4):
        b = col.collect_episode()
        assert b == ep % 3
        snaps.append(snapshot(col, b))
    assert (col.head, col.filled) == (1, 2) and learner.complete_blocks() == [0, 2]
    stale = snapshot(col, 1)
    assert all(np.array_equal(a[1:] if i == 0 else a, b[1:] if i == 0 else b) for i, (a, b) in enumerate(zip(stale, snaps[1])))
    # Episodes of different pool windows may coincide (a deterministic actor, observations that do not tell the windows apart), so the stale block
    # is made unmistakable: everything in it but the next reset row becomes a value no episode holds.  A row drawn from block 1 cannot pass.
    mark = np.float32(-12345.0)
    assert not any(np.any(a == mark) for sn in snaps for a in sn[:3])
    obs1 = stale[0].copy()
    obs1[1:] = mark
    col.obs[1].upload(obs1); col.actions[1].upload(np.full_like(stale[1], mark)); col.reward[1].upload(np.full_like(stale[2], mark))
    same = [(i + 1, j + 1) for i in range(4) for j in range(i) if all(np.array_equal(snaps[i][k], snaps[j][k]) for k in range(3))]
    print(f"ring wrap: episode pairs that coincide in observations, actions and rewards: {same}")
    ring = [(col.obs[b], col.actions[b], col.reward[b], col.done[b]) for b in learner.complete_blocks()]
    seen = check_sample(col, ring, [snaps[3], snaps[2]], B, learner.sample_seed, (0, 1))
    assert not np.array_equal(seen[0], seen[1])
