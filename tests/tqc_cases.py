"""What tests/test_tqc_cpu.py and tests/test_tqc_gpu.py share: the case builder of one TQC batch (SAC's case layout; rows redrawn away from ReLU's
kinks; rewards centred so that the quantile Huber loss is exercised in all four of its regions), the torch restatement of sb3_contrib's
TQC.train() in either precision (autograd, three torch.optim.Adam(eps=1e-8), torch.sort, polyak_update's mul_ / add_), and the comparison under
the project's tolerance idiom (tests/td3_cases.check_arrays).  A plain module.

THE REWARDS.  With raw N(0, 1) rewards -alpha log pi' pushes every target well above the critics' outputs and about 82 % of the pairwise deltas
z_k - q_{j,i} lie above 1: the linear branch of the Huber loss alone.  The stored reward of row b is therefore

    N(0, 1.5) - (1 - done_b) gamma (median_k sorted_k - alpha log pi'_b) + median_{j,i} q_{b,j,i},          rounded to float32,

which centres each row's targets on its current quantiles.  The builder ASSERTS, for B >= 17, that each of the regions delta < -1, -1 <= delta < 0,
0 <= delta <= 1 and delta > 1 holds at least 5 % of the pairwise deltas of the float64 reference (the loss and its gradient are continuous at 0 and
at +-1, so no exclusion is needed there), and, with n_critics >= 2 and drop >= 1, that in at least a quarter of the rows the dropped atoms come
from more than one critic."""
import math

import numpy as np

from tests import sac_cases as sc
from tests.td3_cases import KINK, check_arrays, nonzero_grads  # noqa: F401  (re-exported for the tests)

NETS = sc.NETS
EDGE_NETS = sc.EDGE_NETS
REGION_SHARE = 0.05      # each of the four Huber regions, of the pairwise deltas (B >= 17)
MIXED_DROP_SHARE = 0.25  # rows whose dropped atoms come from more than one critic (n_critics >= 2, drop >= 1)

# (tag, n_critics, n_quantiles, drop, lo, auto, B): the plan's limits and the sort's lane edges (csrc/ev2g_tqc.h: one wavefront per row, at most
# two atoms per lane).  M 125 and M 128 (every lane two atoms) at the largest network, B 1023 and 1024 once each; M 64 / 65, the one-atom /
# two-atom boundary; K 2 and K 1; one atom in all.
EDGE_GRAD_CASES = [("limits", 5, 25, 2, 0.0, True, 1023), ("limits", 2, 64, 0, -1.0, False, 1024),
                   ("lanes", 1, 64, 2, -1.0, True, 37), ("lanes+1", 5, 13, 2, 0.0, False, 37),
                   ("lanes", 2, 3, 2, 0.0, False, 37), ("lanes+1", 1, 3, 2, -1.0, True, 37), ("tiny", 1, 1, 0, -1.0, True, 37)]


BATCHES = (1, 17, 37, 257)
DP = ((11, 5), (63, 20), (162, 50))
QUANTILES = ((2, 25, 2), (1, 25, 2), (5, 25, 2), (2, 64, 0), (3, 7, 1), (1, 1, 0))


def grad_cases():
    """(net, (D, P), (nc, nq, d), lo, auto, B): every network with every (nc, nq, d) -- 18 cases; within a network (D, P) and B step with the
    quantile setting, each network starting one further on, so that each (D, P) meets each network twice and each B at least once, and lo and
    auto take both values on each network.  256-256 with 2 x 25, d 2 runs at (162, 50), the shape the rate tool times.
    tests/test_tqc_cpu.py asserts the coverage."""
    out = []
    for a, net in enumerate(NETS):
        for j, qs in enumerate(QUANTILES):
            out.append((net, DP[(j + a + 2) % 3], qs, (-1.0, 0.0)[j % 2], bool((j // 2 + a) % 2 == 0), BATCHES[(j + a) % 4]))
    return out


def grad_case(net, dp, qs, lo, auto, B):
    return make_case(*dp, net, *qs, B, lo, 0.7, auto, seed=7 + B, first_draw=1000)


def edge_grad_case(tag, nc, nq, drop, lo, auto, B):
    D, _, _, P = EDGE_NETS[tag]
    return make_case(D, P, tag, nc, nq, drop, B, lo, 0.7, auto, seed=7 + B, first_draw=1000, live=True)


def kept(case):
    return case["n_critics"] * (case["n_quantiles"] - case["drop"])


def _row_margin(case, rows):
    """Per row: the smallest |pre-activation| over every ReLU layer that is backpropagated through -- the actor's trunk on s, the critics on
    (s, a~) and on (s, a_pi) (float64)."""
    from ev2gym_amd.sac import sac_actor_forward
    from ev2gym_amd.td3 import _f64, _forward, scale_action
    s = case["obs"][rows].astype(np.float64)
    a = scale_action(case["actions"][rows].astype(np.float64), case["lo"])
    fa = sac_actor_forward(case["actor"], s, case["eps"][rows])
    m = [np.abs(fa.z1).min(1), np.abs(fa.z2).min(1)]
    for c in case["critics"]:
        for x in (np.concatenate([s, a], 1), np.concatenate([s, fa.a], 1)):
            f = _forward(_f64(c), x, False)
            m += [np.abs(f.z1).min(1), np.abs(f.z2).min(1)]
    return np.min(m, axis=0)


def numpy_critic(case):
    """tqc_critic_numpy on the case as it stands: (grads, loss, aux)."""
    from ev2gym_amd.tqc import tqc_critic_numpy
    return tqc_critic_numpy(case["actor"], case["critics"], case["critics"], case["obs"], case["actions"], case["reward"], case["next_obs"], case["done"],
                            case["eps_next"], case["log_ent_coef"], case["lo"], case["gamma"], case["drop"])


def coverage(case):
    """(the four regions' shares of the float64 reference's pairwise deltas, the share of rows whose dropped atoms come from more than one critic
    -- None where nothing is dropped or there is one critic)."""
    aux = numpy_critic(case)[2]
    d = aux.delta
    shares = (float((d < -1.0).mean()), float(((d >= -1.0) & (d < 0.0)).mean()), float(((d >= 0.0) & (d <= 1.0)).mean()), float((d > 1.0).mean()))
    mixed = None
    if case["n_critics"] >= 2 and case["drop"] >= 1:
        owners = aux.order[:, kept(case):] // case["n_quantiles"]
        mixed = float((owners.min(1) != owners.max(1)).mean())
    return shares, mixed


def make_case(D, P, net="64-64", n_critics=2, n_quantiles=25, drop=2, B=37, lo=-1.0, ent_coef=0.7, auto=True, seed=7, noise_seed=11, first_draw=0,
              live=False):
    """_draw_case(seed) under tests/td3_cases.make_case's cap: fewer than a quarter of the rows needed a redraw; with ONE row (a quarter means
    none) or with `live` the first of ten fixed seeds (seed, seed + 1000, ...) that fits is taken.  live (required on edge shapes): every float64
    reference gradient array has a non-zero element; the reference is kept as case["ref64"].  Then the coverage of the Huber loss and of the
    truncation is asserted (module docstring); case["regions"] and case["mixed_drop"] hold the shares."""
    import torch
    for i in range(10 if (B == 1 or live) else 1):
        case = _draw_case(D, P, net, n_critics, n_quantiles, drop, B, lo, ent_coef, auto, seed + 1000 * i, noise_seed, first_draw)
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
    case["regions"], case["mixed_drop"] = coverage(case)
    if B >= 17:
        assert min(case["regions"]) >= REGION_SHARE, f"a Huber region holds less than {REGION_SHARE:.0%} of the deltas: {case['regions']}"
    if case["mixed_drop"] is not None:
        assert case["mixed_drop"] >= MIXED_DROP_SHARE, f"the dropped atoms come from more than one critic in {case['mixed_drop']:.0%} of the rows only"
    return case


def _draw_case(D, P, net, n_critics, n_quantiles, drop, B, lo, ent_coef, auto, seed, noise_seed, first_draw):
    """One batch and the networks of a learner in tests/sac_cases._draw_case's layout: torch-style initial weights, observations in [0, 1], stored
    actions in [lo, 1], `done` mixed, the standard normals of a_pi (draws first_draw + b P + p) and of a' (first_draw + B P + b P + p) from the
    host twin; rows inside KINK of a ReLU kink redrawn; then the centred rewards."""
    from ev2gym_amd.engine import host_normal
    from ev2gym_amd.sac import init_sac_actor_weights
    from ev2gym_amd.tqc import init_tqc_critic_weights
    h1, h2 = sc._hidden(net)
    rng = np.random.default_rng(seed)
    case = dict(D=D, P=P, h=(h1, h2), n_critics=n_critics, n_quantiles=n_quantiles, drop=drop, B=B, lo=float(lo), gamma=0.99, noise_seed=noise_seed,
                first_draw=first_draw, actor=init_sac_actor_weights(D, P, seed, h1, h2),
                critics=[init_tqc_critic_weights(D, P, n_quantiles, seed + 1 + j, h1, h2) for j in range(n_critics)], auto=bool(auto), clamp=False,
                log_ent_coef=float(np.float32(math.log(ent_coef))), target_entropy=-float(P))
    case["obs"] = rng.uniform(0.0, 1.0, (B, D)).astype(np.float32)
    case["actions"] = rng.uniform(lo, 1.0, (B, P)).astype(np.float32)
    noise = rng.normal(0.0, 1.5, B)
    case["next_obs"] = rng.uniform(0.0, 1.0, (B, D)).astype(np.float32)
    case["done"] = (rng.uniform(size=B) < 0.3).astype(np.uint8)
    if B > 1:
        case["done"][:2] = (0, 1)
    case["eps"] = host_normal(B * P, noise_seed, first_draw).reshape(B, P)
    case["eps_next"] = host_normal(B * P, noise_seed, first_draw + B * P).reshape(B, P)
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
    # the centred rewards: from the float64 reference's sorted target atoms and current quantiles (neither depends on the reward)
    case["reward"] = np.zeros(B, np.float32)
    aux = numpy_critic(case)[2]
    alpha = math.exp(case["log_ent_coef"])
    centre = np.median(aux.sorted[:, :kept(case)], axis=1) - alpha * aux.logp_next
    q_mid = np.median(aux.q.transpose(1, 0, 2).reshape(B, -1), axis=1)
    case["reward"] = (noise - (1.0 - case["done"]) * case["gamma"] * centre + q_mid).astype(np.float32)
    return case


# ---- the torch restatement ----
def torch_nets(case, dtype):
    return sc.torch_nets(case, dtype)


def quantile_huber_loss(current, target):
    """sb3_contrib.common.utils.quantile_huber_loss(current [B, nc, nq], target [B, K], sum_over_quantiles=False)."""
    import torch
    nq = current.shape[-1]
    cum_prob = ((torch.arange(nq, dtype=current.dtype) + 0.5) / nq).view(1, 1, -1, 1)
    delta = target[:, None, None, :] - current[:, :, :, None]
    ad = delta.abs()
    huber = torch.where(ad > 1.0, ad - 0.5, delta ** 2 * 0.5)
    return (torch.abs(cum_prob - (delta.detach() < 0).to(current.dtype)) * huber).mean()


def torch_critic_loss(case, actor, critics, critics_t, batch, eps_next, alpha):
    """(critic_loss, z [B, K], log pi') as sb3_contrib writes them."""
    import torch
    s, a, r, s2, d = batch
    with torch.no_grad():
        a2, lp2 = sc.torch_actor(actor, s2, eps_next)
        xn = torch.cat([s2, a2], 1)
        pooled = torch.stack([sc._mlp(c, xn) for c in critics_t], 1).reshape(s.shape[0], -1)
        srt = torch.sort(pooled, dim=1).values[:, :kept(case)]
        z = r[:, None] + (1.0 - d)[:, None] * case["gamma"] * (srt - alpha * lp2[:, None])
    xa = torch.cat([s, a], 1)
    cur = torch.stack([sc._mlp(c, xa) for c in critics], 1)
    return quantile_huber_loss(cur, z), z, lp2


def torch_actor_loss(actor, critics, s, eps, alpha):
    import torch
    a, lp = sc.torch_actor(actor, s, eps)
    xa = torch.cat([s, a], 1)
    qf_pi = torch.stack([sc._mlp(c, xa) for c in critics], 1).mean(dim=2).mean(dim=1)
    return (alpha * lp - qf_pi).mean(), lp


def torch_grads(case, dtype):
    """One staged step (the critics' gradient, then the actor's and log_ent_coef's through the UNCHANGED critics) by autograd: dict of z,
    log_pi_next, log_pi, critic_loss, actor_loss, ent_coef_loss, ent_coef_grad, critic_grads (a list of six per critic), actor_grads, as
    float64 numpy."""
    import torch
    actor, critics = torch_nets(case, dtype)
    batch = sc._batch(case, dtype)
    la = torch.tensor(case["log_ent_coef"], dtype=dtype, requires_grad=True)
    alpha = la.detach().exp()
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    closs, z, lp2 = torch_critic_loss(case, actor, critics, [[a.detach() for a in c] for c in critics], batch, t(case["eps_next"]), alpha)
    cg = torch.autograd.grad(closs, [a for c in critics for a in c])
    aloss, lp = torch_actor_loss(actor, critics, batch[0], t(case["eps"]), alpha)
    ag = torch.autograd.grad(aloss, actor)
    eloss = -(la * (lp.detach() + case["target_entropy"])).mean()
    eg = torch.autograd.grad(eloss, la)[0] if case["auto"] else torch.zeros(())
    n = lambda x: x.detach().double().numpy()  # noqa: E731
    return dict(z=n(z), log_pi_next=n(lp2), log_pi=n(lp), critic_loss=float(closs.detach().double()), actor_loss=float(aloss.detach().double()),
                ent_coef_loss=float(eloss.detach().double()) if case["auto"] else 0.0, ent_coef_grad=float(eg.double()),
                critic_grads=[[n(g) for g in cg[6 * j:6 * j + 6]] for j in range(case["n_critics"])], actor_grads=[n(g) for g in ag])


def torch_loop(case, batches, dtype, target_update_interval=1, lr=3e-4, tau=0.005, grads=False):
    """sb3_contrib's TQC.train() over `batches` (a list of (row indices, eps, eps_next)): per step a dict of the four losses and float64 copies
    of the masters, the target critics and log_ent_coef after the step (grads: also z, both log pi, the gradients and that of log_ent_coef)."""
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
        batch = sc._batch(case, dtype, rows)
        e1, e2 = torch.tensor(np.asarray(eps), dtype=dtype), torch.tensor(np.asarray(eps_next), dtype=dtype)
        alpha = la.detach().exp().clone()
        with torch.no_grad():
            _, lp = sc.torch_actor(actor, batch[0], e1)
        eloss, eg = torch.zeros(()), 0.0
        if case["auto"]:
            eloss = -(la * (lp + case["target_entropy"])).mean()
            opt_e.zero_grad(); eloss.backward(); eg = float(la.grad.double()); opt_e.step()
        closs, z, lp2 = torch_critic_loss(case, actor, critics, critics_t, batch, e2, alpha)
        opt_c.zero_grad(); closs.backward(); opt_c.step()
        cg = [n([a.grad for a in c]) for c in critics] if grads else None
        aloss, _ = torch_actor_loss(actor, critics, batch[0], e1, alpha)
        opt_a.zero_grad(); aloss.backward(); opt_a.step()
        if k % target_update_interval == 0:
            with torch.no_grad():
                for tgt, src in zip([a for c in critics_t for a in c], [a for c in critics for a in c]):
                    tgt.mul_(1.0 - tau)
                    torch.add(tgt, src, alpha=tau, out=tgt)
        step = dict(critic_loss=float(closs.detach().double()), actor_loss=float(aloss.detach().double()), ent_coef_loss=float(eloss.detach().double()),
                    ent_coef=float(alpha.double()), actor=n(actor), critics=[n(c) for c in critics], critics_target=[n(c) for c in critics_t],
                    log_ent_coef=float(la.detach().double()))
        if grads:
            step.update(z=z.double().numpy().copy(), log_pi=lp.double().numpy().copy(), log_pi_next=lp2.double().numpy().copy(), critic_grads=cg,
                        actor_grads=n([a.grad for a in actor]), ent_coef_grad=eg)
        out.append(step)
    return out


loop_batches = sc.loop_batches


# ---- rows for the sort: crafted pools [B, M] as target-critic atoms [nc, B, nq] ----
SORT_KINDS = ("random", "equal", "reversed", "sorted", "ties", "zeros", "done")
SORT_SHAPES = ((1, 1, 0), (2, 1, 0), (1, 63, 2), (1, 64, 2), (2, 32, 1), (5, 13, 2), (1, 64, 0), (5, 25, 2), (2, 64, 0), (2, 64, 3))   # (nc, nq, drop): M 1, 2, 63, 64, 64, 65, 64, 125, 128, 128


def sort_rows(kind, nc, nq, B, seed=0):
    """(tq [nc, B, nq], log pi' [B], reward [B], done [B]) float32 / uint8.  equal: one value per row; reversed / sorted: the pool descending /
    ascending; ties: eight distinct values, each met in every critic; zeros: +0 and -0 mixed with a few other values; done: all 1."""
    rng = np.random.default_rng(seed + 17 * nc + nq)
    M = nc * nq
    pool = rng.normal(0.0, 3.0, (B, M)).astype(np.float32)
    if kind == "equal":
        pool[:] = pool[:, :1]
    elif kind == "reversed":
        pool = -np.sort(-pool, axis=1)
    elif kind == "sorted":
        pool = np.sort(pool, axis=1)
    elif kind == "ties":
        pool = rng.normal(0.0, 3.0, 8).astype(np.float32)[rng.integers(0, 8, (B, M))]
    elif kind == "zeros":
        pool = np.array([0.0, -0.0, 0.0, -0.0, 1.5, -2.0], np.float32)[rng.integers(0, 6, (B, M))]
    tq = np.ascontiguousarray(pool.reshape(B, nc, nq).transpose(1, 0, 2))
    done = np.ones(B, np.uint8) if kind == "done" else (rng.uniform(size=B) < 0.3).astype(np.uint8)
    return tq, rng.normal(-5.0, 3.0, B).astype(np.float32), rng.normal(0.0, 1.0, B).astype(np.float32), done
