"""What tests/test_sac_cpu.py and tests/test_sac_gpu.py share: the case builder of one SAC batch (rows redrawn away from ReLU's kinks and from the
argmin's kink between the two critics), the torch restatement of SB3's SAC.train() in either precision (autograd, three torch.optim.Adam(eps=1e-8),
polyak_update's mul_ / add_, the reduced Gaussian term of ev2gym_amd/sac.py), and the comparison under the project's tolerance idiom
(tests/td3_cases.check_arrays).  A plain module."""
import math

import numpy as np

from tests.td3_cases import KINK, SATURATED, check_arrays, check_ring_wrap, grad_tol, nonzero_grads, saturated_ports  # noqa: F401  (re-exported for the tests)

NETS = {"256-256": (256, 256), "64-64": (64, 64), "33-17": (33, 17)}
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
# The plan's limits and the head's lane edges (csrc/ev2g_sac.h: eight lanes per row, lane j takes ports j, j + 8, ...; the collection actor pads
# inputs to k1 = ceil8(D) and ports to n3 = ceil32(P)): tag -> (D, h1, h2, P).  A table of its own: the GPU module's _grad_cases() cycles over NETS.
#   limits   every plan maximum; n3 == P, so no padded port; lane 0's (every lane's) eighth port
#   lanes    one port per head lane; k1 == D
#   lanes+1  lane 0 alone takes a second port; k1 16 with 7 zero columns
#   eighth   lane 0 alone takes an eighth port (P 57 > 56)
#   tiny     seven idle head lanes; k1 8 with 7 zero columns
EDGE_NETS = {"limits": (192, 256, 256, 64), "lanes": (8, 16, 16, 8), "lanes+1": (9, 33, 17, 9), "eighth": (63, 64, 64, 57), "tiny": (1, 5, 2, 1)}


# (tag, n_critics, lo, auto, B): B in {1, 37, 1023, 1024} at limits and {37, 1024} elsewhere; n_critics, lo and auto are spread so that each
# value meets each network, and both large batches at limits run two critics.
EDGE_GRAD_CASES = [("limits", 1, 0.0, True, 1), ("limits", 1, -1.0, False, 37), ("limits", 2, -1.0, False, 1023), ("limits", 2, 0.0, True, 1024),
                   ("lanes", 2, -1.0, True, 37), ("lanes", 1, 0.0, False, 1024), ("lanes+1", 1, 0.0, False, 37), ("lanes+1", 2, -1.0, True, 1024),
                   ("eighth", 2, 0.0, False, 37), ("eighth", 1, -1.0, True, 1024), ("tiny", 1, -1.0, True, 37), ("tiny", 2, 0.0, False, 1024)]
# (net, (D, P), n_critics, lo, auto, B) with a saturated actor
SATURATED_GRAD_CASES = [("64-64", (63, 20), 2, -1.0, True, 37), ("limits", (192, 64), 2, 0.0, True, 257)]
ACT_EDGE_CASES = [("limits", 0.0), ("lanes+1", -1.0), ("tiny", 0.0)]   # (tag, lo) of the collection actor's cases off NETS


def edge_grad_case(tag, n_critics, lo, auto, B):
    return edge_case(tag, n_critics, B, lo, 0.7, auto, seed=7 + B, first_draw=1000)


def saturated_grad_case(net, dp, n_critics, lo, auto, B):
    return make_case(*dp, net, n_critics, B, lo, 0.7, auto, seed=7 + B, first_draw=1000, saturate=True, live=True)


def act_case(net, dp, lo, saturate=False):
    """the collection actor's case (70 rows; the clamped log_std columns need three ports)"""
    return make_case(*dp, net, 1, 70, lo, 0.7, True, clamp=dp[1] >= 3, seed=3, saturate=saturate)


def _hidden(net):
    return NETS[net] if net in NETS else EDGE_NETS[net][1:3]


def edge_case(tag, *args, **kw):
    """make_case on a row of EDGE_NETS, with the live-gradient condition."""
    D, _, _, P = EDGE_NETS[tag]
    return make_case(D, P, tag, *args, live=True, **kw)


def _row_margin(case, rows):
    """Per row: the smallest |pre-activation| over every ReLU layer that is backpropagated through -- the actor's trunk on s, the critics on
    (s, a~) and on (s, a_pi) -- and, with two critics, |Q_0 - Q_1|(s, a_pi), the argmin's kink (float64)."""
    from ev2gym_amd.sac import sac_actor_forward
    from ev2gym_amd.td3 import _f64, _forward, scale_action
    s = case["obs"][rows].astype(np.float64)
    a = scale_action(case["actions"][rows].astype(np.float64), case["lo"])
    fa = sac_actor_forward(case["actor"], s, case["eps"][rows])
    m = [np.abs(fa.z1).min(1), np.abs(fa.z2).min(1)]
    q = []
    for c in case["critics"]:
        for x in (np.concatenate([s, a], 1), np.concatenate([s, fa.a], 1)):
            f = _forward(_f64(c), x, False)
            m += [np.abs(f.z1).min(1), np.abs(f.z2).min(1)]
        q.append(f.out[:, 0])
    if len(q) == 2:
        m.append(np.abs(q[0] - q[1]))
    return np.min(m, axis=0)


def make_case(D, P, net="64-64", n_critics=2, B=37, lo=-1.0, ent_coef=0.7, auto=True, clamp=False, seed=7, noise_seed=11, first_draw=0, saturate=False,
              live=False):
    """_draw_case(seed), asserting that fewer than a quarter of the rows needed a redraw.  With ONE row a quarter means none: only then the first
    of ten fixed seeds (seed, seed + 1000, ...) that needs no redraw is taken.  case["seeds_skipped"] says how many seeds were passed over.

    live (the EDGE_NETS and the saturated cases): every float64 reference gradient array must also have a non-zero element
    (tests/td3_cases.nonzero_grads: a dead ReLU in a narrow network zeroes whole arrays), and a seed that misses that or the cap is passed over
    at any B, again among the ten fixed seeds.  The float64 reference is kept as case["ref64"]."""
    import torch
    for i in range(10 if (B == 1 or live) else 1):
        case = _draw_case(D, P, net, n_critics, B, lo, ent_coef, auto, clamp, seed + 1000 * i, noise_seed, first_draw, saturate)
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
    return case


def _draw_case(D, P, net, n_critics, B, lo, ent_coef, auto, clamp, seed, noise_seed, first_draw, saturate=False):
    """One batch and the networks of a learner: torch-style initial weights, observations in [0, 1], stored actions in [lo, 1], rewards of both
    signs, `done` mixed, the standard normals of a_pi (draws first_draw + b P + p) and of a' (first_draw + B P + b P + p) from the host twin.
    clamp: log_std bias 0 is +3 and bias 1 is -25, so those two columns are clamped for every row (asserted).
    saturate: the bias of mu of every second port is moved by +12, -12, +12, ... before the redraws, so that |mu| >= 10 in float64 on those
    ports for every row of obs and next_obs (asserted): a = +-1 to float32 and log(1 - a^2 + 1e-6) sits at its floor wherever the noise does not
    pull u back.  case["share_at_1"]: the share of a_pi and a' elements that are +-1 once rounded to float32."""
    from ev2gym_amd.engine import host_normal
    from ev2gym_amd.sac import init_sac_actor_weights, sac_actor_forward
    from ev2gym_amd.td3 import init_critic_weights
    h1, h2 = _hidden(net)
    rng = np.random.default_rng(seed)
    actor = init_sac_actor_weights(D, P, seed, h1, h2)
    if saturate:
        ports, sign = saturated_ports(P)
        actor[5][ports] += (SATURATED * sign).astype(np.float32)
    if clamp:
        assert P >= 3
        actor[7][0], actor[7][1] = 3.0, -25.0
    case = dict(D=D, P=P, h=(h1, h2), n_critics=n_critics, B=B, lo=float(lo), gamma=0.99, noise_seed=noise_seed, first_draw=first_draw, actor=actor,
                critics=[init_critic_weights(D, P, seed + 1 + j, h1, h2) for j in range(n_critics)], auto=bool(auto), clamp=bool(clamp),
                log_ent_coef=float(np.float32(math.log(ent_coef))), target_entropy=-float(P))
    case["obs"] = rng.uniform(0.0, 1.0, (B, D)).astype(np.float32)
    case["actions"] = rng.uniform(lo, 1.0, (B, P)).astype(np.float32)
    case["reward"] = rng.normal(0.0, 1.0, B).astype(np.float32)
    case["next_obs"] = rng.uniform(0.0, 1.0, (B, D)).astype(np.float32)
    case["done"] = (rng.uniform(size=B) < 0.3).astype(np.uint8)
    if B > 1:
        case["done"][:2] = (0, 1)
    case["eps"] = host_normal(B * P, noise_seed, first_draw).reshape(B, P)
    case["eps_next"] = host_normal(B * P, noise_seed, first_draw + B * P).reshape(B, P)
    if n_critics == 2 and B > 1:
        # torch-style critics differ mostly by their output bias, and one of them would be every row's argmin: critic 1's output bias is moved by the
        # middle of the batch's Q_0 - Q_1 on (s, a_pi), so that each critic is the argmin of about half the rows and the selector is exercised
        from ev2gym_amd.td3 import _f64, _forward
        xa = np.concatenate([case["obs"].astype(np.float64), sac_actor_forward(actor, case["obs"], case["eps"]).a], 1)
        q = [_forward(_f64(c), xa, False).out[:, 0] for c in case["critics"]]
        gap = np.sort(q[0] - q[1])
        case["critics"][1][5] = (case["critics"][1][5] + np.float32(0.5 * (gap[B // 2 - 1] + gap[B // 2]))).astype(np.float32)   # (between two rows' gaps: on no row's kink)
    redrawn = np.zeros(B, bool)
    for _ in range(50):
        bad = np.nonzero(_row_margin(case, np.arange(B)) < KINK)[0]
        if bad.size == 0:
            break
        redrawn[bad] = True
        case["obs"][bad] = rng.uniform(0.0, 1.0, (bad.size, D)).astype(np.float32)
        case["actions"][bad] = rng.uniform(lo, 1.0, (bad.size, P)).astype(np.float32)
    assert _row_margin(case, np.arange(B)).min() >= KINK, "a row still sits on a kink"
    case["redrawn"] = int(redrawn.sum())
    if clamp:
        for x, e in ((case["obs"], case["eps"]), (case["next_obs"], case["eps_next"])):
            raw = sac_actor_forward(actor, x, e).raw
            assert (raw[:, 0] > 2.0).all() and (raw[:, 1] < -20.0).all() and (np.abs(raw[:, 2:]) < 2.0).all(), "the clamp case's columns"
    if saturate:
        ports, at_1 = saturated_ports(P)[0], []
        for x, e in ((case["obs"], case["eps"]), (case["next_obs"], case["eps_next"])):
            f = sac_actor_forward(actor, x, e)
            assert np.abs(f.mu[:, ports]).min() >= 10.0, "a saturated port's mu is inside 10"
            at_1.append(np.abs(f.a.astype(np.float32)) == 1.0)
        case["share_at_1"] = float(np.mean(at_1))
    return case


def torch_nets(case, dtype):
    import torch
    mk = lambda ws: [torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(True) for a in ws]  # noqa: E731
    return mk(case["actor"]), [mk(c) for c in case["critics"]]


def _mlp(w, x):
    import torch
    F = torch.nn.functional
    return F.linear(torch.relu(F.linear(torch.relu(F.linear(x, w[0], w[1])), w[2], w[3])), w[4], w[5])


def torch_actor(w, s, eps, literal=False, mixed=False):
    """(a, log pi) of the squashed Gaussian.  literal: SB3's Normal(mu, sigma).log_prob(u) instead of the reduced Gaussian term.
    mixed: the precision split csrc/ev2g_sac.h states for the device -- the networks in the tensors' own precision (float32), the head in float64
    from mu, the raw log_std and eps as they stand, a and log pi rounded back once; autograd flows through the casts.  The yardstick of the
    saturated cases, where plain float32 forms 1 - a^2 in float32 and its own error exceeds what it is meant to measure."""
    import torch
    F = torch.nn.functional
    h = torch.relu(F.linear(torch.relu(F.linear(s, w[0], w[1])), w[2], w[3]))
    mu, raw = F.linear(h, w[4], w[5]), F.linear(h, w[6], w[7])
    dtype = mu.dtype
    if mixed:
        mu, raw, eps = mu.double(), raw.double(), eps.double()
    ls = torch.clamp(raw, -20.0, 2.0)
    u = mu + ls.exp() * eps
    a = torch.tanh(u)
    gauss = torch.distributions.Normal(mu, ls.exp()).log_prob(u) if literal else -0.5 * eps * eps - ls - HALF_LOG_2PI
    lp = gauss.sum(1) - torch.log(1.0 - a * a + 1e-6).sum(1)
    return a.to(dtype), lp.to(dtype)


def _batch(case, dtype, rows=None):
    import torch
    sl = slice(None) if rows is None else rows
    t = lambda a: torch.tensor(np.asarray(a)[sl], dtype=dtype)  # noqa: E731
    s, a, r, s2, d = t(case["obs"]), t(case["actions"]), t(case["reward"]), t(case["next_obs"]), t(case["done"])
    if case["lo"] == 0.0:
        a = 2.0 * a - 1.0
    return s, a, r, s2, d


def torch_critic_loss(case, actor, critics, critics_t, batch, eps_next, alpha, literal=False, mixed=False):
    """(critic_loss, y, log pi') as SB3 writes them."""
    import torch
    s, a, r, s2, d = batch
    with torch.no_grad():
        a2, lp2 = torch_actor(actor, s2, eps_next, literal, mixed)
        tq = torch.cat([_mlp(c, torch.cat([s2, a2], 1)) for c in critics_t], 1).min(1).values
        y = r + (1.0 - d) * case["gamma"] * (tq - alpha * lp2)
    xa = torch.cat([s, a], 1)
    return 0.5 * sum(torch.nn.functional.mse_loss(_mlp(c, xa)[:, 0], y) for c in critics), y, lp2


def torch_actor_loss(actor, critics, s, eps, alpha, literal=False, mixed=False):
    import torch
    a, lp = torch_actor(actor, s, eps, literal, mixed)
    q = torch.cat([_mlp(c, torch.cat([s, a], 1)) for c in critics], 1).min(1).values
    return (alpha * lp - q).mean(), lp


def torch_grads(case, dtype, literal=False, mixed=False):
    """One staged step (the critics' gradient, then the actor's and log_ent_coef's through the UNCHANGED critics) by autograd: dict of y,
    log_pi_next, log_pi, critic_loss, actor_loss, ent_coef_loss, ent_coef_grad, critic_grads (a list of six per critic), actor_grads, as
    float64 numpy."""
    import torch
    actor, critics = torch_nets(case, dtype)
    batch = _batch(case, dtype)
    la = torch.tensor(case["log_ent_coef"], dtype=dtype, requires_grad=True)
    alpha = la.detach().exp()
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    closs, y, lp2 = torch_critic_loss(case, actor, critics, [[a.detach() for a in c] for c in critics], batch, t(case["eps_next"]), alpha, literal, mixed)
    cg = torch.autograd.grad(closs, [a for c in critics for a in c])
    aloss, lp = torch_actor_loss(actor, critics, batch[0], t(case["eps"]), alpha, literal, mixed)
    ag = torch.autograd.grad(aloss, actor)
    eloss = -(la * (lp.detach() + case["target_entropy"])).mean()
    eg = torch.autograd.grad(eloss, la)[0] if case["auto"] else torch.zeros(())
    n = lambda x: x.detach().double().numpy()  # noqa: E731
    return dict(y=n(y), log_pi_next=n(lp2), log_pi=n(lp), critic_loss=float(closs.detach().double()), actor_loss=float(aloss.detach().double()),
                ent_coef_loss=float(eloss.detach().double()) if case["auto"] else 0.0, ent_coef_grad=float(eg.double()),
                critic_grads=[[n(g) for g in cg[6 * j:6 * j + 6]] for j in range(case["n_critics"])], actor_grads=[n(g) for g in ag])


def torch_loop(case, batches, dtype, target_update_interval=1, lr=3e-4, tau=0.005):
    """SB3's SAC.train() over `batches` (a list of (row indices, eps, eps_next)): per step a dict of the four losses and float64 copies of the
    masters, the target critics and log_ent_coef after the step."""
    import torch
    actor, critics = torch_nets(case, dtype)
    critics_t = [[a.detach().clone() for a in c] for c in critics]
    la = torch.tensor(case["log_ent_coef"], dtype=dtype, requires_grad=True)
    opt_a = torch.optim.Adam(actor, lr=lr, eps=1e-8)
    opt_c = torch.optim.Adam([a for c in critics for a in c], lr=lr, eps=1e-8)
    opt_e = torch.optim.Adam([la], lr=lr, eps=1e-8)
    out = []
    n = lambda ws: [a.detach().double().numpy().copy() for a in ws]  # noqa: E731
    for k, (rows, eps, eps_next) in enumerate(batches, 1):
        batch = _batch(case, dtype, rows)
        e1, e2 = torch.tensor(np.asarray(eps), dtype=dtype), torch.tensor(np.asarray(eps_next), dtype=dtype)
        alpha = la.detach().exp().clone()
        with torch.no_grad():
            _, lp = torch_actor(actor, batch[0], e1)
        eloss = torch.zeros(())
        if case["auto"]:
            eloss = -(la * (lp + case["target_entropy"])).mean()
            opt_e.zero_grad(); eloss.backward(); opt_e.step()
        closs, _, _ = torch_critic_loss(case, actor, critics, critics_t, batch, e2, alpha)
        opt_c.zero_grad(); closs.backward(); opt_c.step()
        aloss, _ = torch_actor_loss(actor, critics, batch[0], e1, alpha)
        opt_a.zero_grad(); aloss.backward(); opt_a.step()
        if k % target_update_interval == 0:
            with torch.no_grad():
                for tgt, src in zip([a for c in critics_t for a in c], [a for c in critics for a in c]):
                    tgt.mul_(1.0 - tau)
                    torch.add(tgt, src, alpha=tau, out=tgt)
        out.append(dict(critic_loss=float(closs.detach().double()), actor_loss=float(aloss.detach().double()), ent_coef_loss=float(eloss.detach().double()),
                        ent_coef=float(alpha.double()), actor=n(actor), critics=[n(c) for c in critics], critics_target=[n(c) for c in critics_t],
                        log_ent_coef=float(la.detach().double())))
    return out


def loop_batches(case, n_steps, B, seed=5):
    """n_steps batches of B rows of the case (with replacement across steps) and their draws: the learner's stream from the case's first_draw,
    2 B P draws per update."""
    from ev2gym_amd.engine import host_normal
    rng = np.random.default_rng(seed)
    P, d = case["P"], case["first_draw"]
    out = []
    for _ in range(n_steps):
        rows = rng.choice(case["B"], B, replace=False)
        out.append((rows, host_normal(B * P, case["noise_seed"], d).reshape(B, P), host_normal(B * P, case["noise_seed"], d + B * P).reshape(B, P)))
        d += 2 * B * P
    return out


def torch_act(actor, x, eps, dtype, lo=-1.0):
    """The collection actor on rows x with the standard normals eps (zeros: deterministic) in `dtype`: (env action in [lo, 1], mu, raw log_std,
    log pi) as float64 numpy."""
    import torch
    F = torch.nn.functional
    w = [torch.tensor(np.asarray(a), dtype=dtype) for a in actor]
    s, e = torch.tensor(np.asarray(x), dtype=dtype), torch.tensor(np.asarray(eps), dtype=dtype)
    with torch.no_grad():
        h = torch.relu(F.linear(torch.relu(F.linear(s, w[0], w[1])), w[2], w[3]))
        mu, raw = F.linear(h, w[4], w[5]), F.linear(h, w[6], w[7])
        ls = torch.clamp(raw, -20.0, 2.0)
        a = torch.tanh(mu + ls.exp() * e)
        lp = (-0.5 * e * e - ls - HALF_LOG_2PI).sum(1) - torch.log(1.0 - a * a + 1e-6).sum(1)
        env = 0.5 * (a + 1.0) if float(lo) == 0.0 else a
    return [t.double().numpy() for t in (env, mu, raw, lp)]
