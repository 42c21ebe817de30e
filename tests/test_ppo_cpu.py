"""The PPO learner's arithmetic without a GPU (ev2gym_amd/ppo.py, csrc/ev2g_ppo.h's host twins, the host-only plan of ev2g_policy_host.h):

  * `ppo_minibatch_numpy` (float64, analytic backprop) against torch float64 autograd of the loss written with torch.min / torch.clamp /
    F.mse_loss / the unbiased std, to 1e-10 of each array's largest magnitude;
  * `adam_numpy` + `clip_grad_norm_numpy` against torch.optim.Adam and clip_grad_norm_ in float64, five steps, to 1e-12;
  * the host twins `ev2g_host_adam` and `ev2g_host_ppo_head` (the device's element functions compiled for the host) against the float64
    references by the project's tolerance idiom: d32 = the largest deviation of the same computation in torch-CPU float32 from the float64
    reference; the twin gets 4 d32 + 4 * 2^-23 * s, s = max(1, |y|) for parameters and statistics, the array's largest reference magnitude for
    gradients.  Every figure is printed before it is asserted;
  * `ev2g_ppo_query`'s accepted and refused networks, and the Python-side refusals.

The clip and the ReLU make the gradient discontinuous, so the cases are CONSTRUCTED to sit away from the branches: old_log_prob = lp64 + o with
o cycling through {-0.5, -0.05, +0.05, +0.5} (ratios 0.607, 0.951, 1.051, 1.649 against a clip range of 0.2) and advantages of both signs;
a ReLU case takes the first of ten fixed seeds for which no float64 pre-activation has |z| < 1e-5.  The helpers are shared with
tests/test_ppo_gpu.py."""
import os

import numpy as np
import pytest

EPS32 = 2.0 ** -23
OFFSETS = np.array([-0.5, -0.05, 0.05, 0.5])
RELU_SEEDS = (101, 102, 103, 104, 105, 106, 107, 108, 109, 110)
CLIP = 0.2


def _record(line):
    """A figure of this run: printed, and appended to the file EV2G_PPO_RECORD names when it is set (how the numerics part of
    profiles/r18_ppo_learner.txt is taken; an ordinary run of the suite writes nothing into the tree)."""
    print(line)
    path = os.environ.get("EV2G_PPO_RECORD")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def _rows(D, P, h, v, activation, n_rows, seed):
    """Weights, log_std and n_rows random rows: observations in [0, 1], actions, advantages of both signs, returns, and old_log_prob = the
    float64 log-probability + the cycling offset.  Everything float32, as the device holds it."""
    from ev2gym_amd.onpolicy import init_ac_weights
    from ev2gym_amd.ppo import ppo_minibatch_numpy
    rng = np.random.default_rng(seed)
    w = init_ac_weights(D, P, seed=seed, h=h, v=v)
    log_std = rng.uniform(-0.7, 0.0, P).astype(np.float32)
    obs = rng.uniform(0.0, 1.0, (n_rows, D)).astype(np.float32)
    actions = rng.normal(0.0, 0.6, (n_rows, P)).astype(np.float32)
    adv = rng.normal(0.0, 1.0, n_rows).astype(np.float32)
    ret = rng.normal(0.0, 1.0, n_rows).astype(np.float32)
    _, _, aux = ppo_minibatch_numpy(w, log_std, obs, actions, np.zeros(n_rows), adv, ret, np.arange(n_rows), activation=activation)
    old = (aux["lp"] + OFFSETS[np.arange(n_rows) % 4]).astype(np.float32)
    zmin = min(float(np.abs(z).min()) for z in aux["z"])
    return dict(weights=w, log_std=log_std, obs=obs, actions=actions, old_log_prob=old, advantages=adv, returns=ret, activation=activation,
                zmin=zmin, D=D, P=P, h=h, v=v)


def make_case(D, P, h=(64, 64), v=(64, 64), activation="tanh", n_rows=600, seed=7):
    """The rows of a gradient case.  ReLU: the first of RELU_SEEDS whose float64 pre-activations all keep |z| >= 1e-5 (fails if none does)."""
    if activation != "relu":
        return _rows(D, P, h, v, activation, n_rows, seed)
    for s in RELU_SEEDS:
        c = _rows(D, P, h, v, activation, n_rows, s)
        if c["zmin"] >= 1e-5:
            return c
    raise AssertionError("no seed of RELU_SEEDS keeps every float64 pre-activation away from 0")


def check_branches(aux):
    """Asserted on the float64 reference: all four (sign of the advantage, clipped?) combinations occur."""
    pos, clipped = aux["adv"] >= 0.0, ~aux["open"]
    seen = {(bool(p), bool(c)) for p, c in zip(pos, clipped)}
    assert seen == {(True, True), (True, False), (False, True), (False, False)}, seen
    assert (np.minimum(np.abs(aux["ratio"] - (1.0 - CLIP)), np.abs(aux["ratio"] - (1.0 + CLIP))) > 0.04).all()   # none near a boundary


def reference(case, idx, clip=CLIP, **cfg):
    from ev2gym_amd.ppo import ppo_minibatch_numpy
    return ppo_minibatch_numpy(case["weights"], case["log_std"], case["obs"], case["actions"], case["old_log_prob"], case["advantages"],
                               case["returns"], idx, activation=case["activation"], clip_range=clip, **cfg)


def torch_params(case, dtype):
    import torch
    return [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in list(case["weights"]) + [case["log_std"]]]


def torch_loss(params, case, idx, dtype, vf_coef=0.5, ent_coef=0.0, normalize_advantage=True, clip=CLIP):
    """PPO.train()'s loss of one minibatch as SB3 writes it, in `dtype` on the CPU: (loss, the six statistics as tensors)."""
    import torch
    F = torch.nn.functional
    act = torch.tanh if case["activation"] == "tanh" else torch.relu
    t = lambda k: torch.tensor(case[k][np.asarray(idx)], dtype=dtype)  # noqa: E731
    x, a, old, adv, ret = t("obs"), t("actions"), t("old_log_prob"), t("advantages"), t("returns")
    p = params
    mu = F.linear(act(F.linear(act(F.linear(x, p[0], p[1])), p[2], p[3])), p[8], p[9])
    v = F.linear(act(F.linear(act(F.linear(x, p[4], p[5])), p[6], p[7])), p[10], p[11]).flatten()
    dist = torch.distributions.Normal(mu, torch.ones_like(mu) * p[12].exp())
    lp, entropy = dist.log_prob(a).sum(dim=1), dist.entropy().sum(dim=1)
    if normalize_advantage and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old)
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vl = F.mse_loss(ret, v)
    el = -torch.mean(entropy)
    loss = pl + ent_coef * el + vf_coef * vl
    with torch.no_grad():
        lr = lp - old
        kl = torch.mean((torch.exp(lr) - 1) - lr)
        cf = torch.mean((torch.abs(ratio - 1) > clip).to(dtype))
    return loss, [pl, vl, el, loss, kl, cf]


def torch_grads(case, idx, dtype, **cfg):
    """(the thirteen gradients, the six statistics) of one minibatch by torch autograd in `dtype`, as float64 numpy arrays"""
    params = torch_params(case, dtype)
    loss, stats = torch_loss(params, case, idx, dtype, **cfg)
    loss.backward()
    return [p.grad.numpy().astype(np.float64) for p in params], np.array([float(s.detach()) for s in stats])


def torch_train(case, minibatches, dtype, lr=3e-4, max_grad_norm=0.5, lrs=None, **cfg):
    """The loop a user has today: clip_grad_norm_ and torch.optim.Adam(eps=1e-5) over `minibatches` (lrs: the rate of each step, set in the
    optimiser's param group before it, as a schedule does; cfg may carry `clip`).  (final parameters as float64 numpy, the statistics [n, 6],
    the gradient norms before clipping)"""
    import torch
    params = torch_params(case, dtype)
    opt = torch.optim.Adam(params, lr=lr, eps=1e-5)
    stats, norms = [], []
    for k, idx in enumerate(minibatches):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        loss, st = torch_loss(params, case, idx, dtype, **cfg)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_grad_norm)))
        opt.step()
        stats.append([float(s.detach()) for s in st])
    return [p.detach().numpy().astype(np.float64) for p in params], np.array(stats), norms


def grad_tol(ref, d32):
    return 4.0 * d32 + 4.0 * EPS32 * float(np.abs(ref).max())


def value_tol(ref, d32):
    return 4.0 * d32 + 4.0 * EPS32 * np.maximum(1.0, np.abs(ref))


# ---- ppo_minibatch_numpy against torch float64 autograd ----
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_numpy_reference_matches_torch_float64_autograd(activation, normalize, ent_coef, B):
    import torch
    case = make_case(11, 5, h=(9, 6), v=(7, 10), activation=activation, n_rows=80)
    assert case["zmin"] >= 1e-5 or activation == "tanh"
    idx = np.random.default_rng(B).integers(0, 80, B)
    cfg = dict(vf_coef=0.5, ent_coef=ent_coef, normalize_advantage=normalize)
    grads, stats, aux = reference(case, idx, **cfg)
    if B > 1:
        check_branches(aux)
    tg, ts = torch_grads(case, idx, torch.float64, **cfg)
    for name, g, t in zip(range(13), grads, tg):
        assert g.shape == t.shape, name
        assert np.abs(g - t).max() <= 1e-10 * max(np.abs(t).max(), 1e-300), name
    assert (np.abs(stats - ts) <= 1e-10 * np.maximum(1.0, np.abs(ts))).all()


def test_adam_and_clip_numpy_match_torch_float64():
    import torch
    from ev2gym_amd.ppo import adam_numpy, clip_grad_norm_numpy
    rng = np.random.default_rng(3)
    shapes = [(6, 4), (6,), (3, 6), (3,)]
    theta = [rng.normal(size=s) for s in shapes]
    m, v = [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    params = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in theta]
    opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5)
    for t in range(1, 6):
        g = [rng.normal(size=s) * (3.0 if t % 2 else 0.01) for s in shapes]   # the clip binds on odd steps only
        for p, gi in zip(params, g):
            p.grad = torch.tensor(gi)
        norm_t = float(torch.nn.utils.clip_grad_norm_(params, 0.5))
        opt.step()
        gc, norm = clip_grad_norm_numpy(g, 0.5)
        assert (norm > 0.5) == bool(t % 2) and abs(norm - norm_t) <= 1e-12 * norm_t
        for i in range(len(shapes)):
            theta[i], m[i], v[i] = adam_numpy(theta[i], m[i], v[i], gc[i], t, lr=3e-4, eps=1e-5)
            ref = params[i].detach().numpy()
            assert np.abs(theta[i] - ref).max() <= 1e-12 * np.abs(ref).max(), (t, i)


# ---- the host twins ----
def test_host_adam_against_adam_numpy():
    import torch
    from ev2gym_amd.engine import host_adam
    from ev2gym_amd.ppo import adam_numpy
    rng = np.random.default_rng(5)
    n = 4099
    theta0 = rng.normal(0.0, 0.3, n).astype(np.float32)
    gs = [(rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32) for _ in range(5)]
    th64, m64, v64 = theta0.astype(np.float64), np.zeros(n), np.zeros(n)
    th, m, v = theta0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    p32 = torch.tensor(theta0, requires_grad=True)
    opt = torch.optim.Adam([p32], lr=3e-4, eps=1e-5)
    for t, g in enumerate(gs, start=1):
        th64, m64, v64 = adam_numpy(th64, m64, v64, g, t, lr=3e-4, eps=1e-5)
        host_adam(th, m, v, g, t, lr=3e-4, eps=1e-5)
        p32.grad = torch.tensor(g)
        opt.step()
        d32 = float(np.abs(p32.detach().numpy() - th64).max())
        dev = np.abs(th - th64)
        _record(f"HOST_ADAM step {t}: d32 {d32:.3e}  |theta - f64| {dev.max():.3e} (tol {value_tol(th64, d32).min():.3e})")
        assert (dev <= value_tol(th64, d32)).all()
    assert np.abs(m - m64).max() <= 8 * EPS32 * np.abs(m64).max() and np.abs(v - v64).max() <= 8 * EPS32 * np.abs(v64).max()


@pytest.mark.parametrize("normalize,ent_coef", [(True, 0.0), (False, 0.01)])
def test_host_ppo_head_against_the_float64_head(normalize, ent_coef):
    import torch
    from ev2gym_amd.engine import host_ppo_head
    B, P = 97, 20
    rng = np.random.default_rng(9)
    mean = rng.normal(0.0, 0.5, (B, P)).astype(np.float32)
    value = rng.normal(0.0, 1.0, B).astype(np.float32)
    actions = (mean + rng.normal(0.0, 0.6, (B, P))).astype(np.float32)
    log_std = rng.uniform(-0.7, 0.0, P).astype(np.float32)
    adv, ret = rng.normal(0.0, 1.0, B).astype(np.float32), rng.normal(0.0, 1.0, B).astype(np.float32)

    def head(dtype, old):
        mu, v, ls = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (mean, value, log_std))
        dist = torch.distributions.Normal(mu, torch.ones_like(mu) * ls.exp())
        lp, ent = dist.log_prob(torch.tensor(actions, dtype=dtype)).sum(1), dist.entropy().sum(1)
        if old is None:
            return lp.detach().numpy()
        A = torch.tensor(adv, dtype=dtype)
        if normalize:
            A = (A - A.mean()) / (A.std() + 1e-8)
        lr = lp - torch.tensor(old, dtype=dtype)
        r = torch.exp(lr)
        pl = -torch.min(A * r, A * torch.clamp(r, 1 - CLIP, 1 + CLIP)).mean()
        vl = torch.nn.functional.mse_loss(torch.tensor(ret, dtype=dtype), v)
        el = -ent.mean()
        loss = pl + ent_coef * el + 0.5 * vl
        loss.backward()
        st = [pl, vl, el, loss, ((r - 1) - lr).mean(), (torch.abs(r - 1) > CLIP).to(dtype).mean()]
        return [mu.grad.numpy().astype(np.float64), v.grad.numpy().astype(np.float64), ls.grad.numpy().astype(np.float64),
                np.array([float(s.detach()) for s in st])]

    old = (head(torch.float64, None) + OFFSETS[np.arange(B) % 4]).astype(np.float32)
    ref, y32 = head(torch.float64, old), head(torch.float32, old)
    got = host_ppo_head(mean, value, actions, log_std, old, adv, ret, clip_range=CLIP, vf_coef=0.5, ent_coef=ent_coef, normalize_advantage=normalize)
    for name, r, y, g in zip(("d_mean", "d_value", "d_log_std"), ref, y32, got):
        d32, dev = float(np.abs(y - r).max()), float(np.abs(g - r).max())
        _record(f"HOST_HEAD normalize {normalize} {name}: d32 {d32:.3e}  |twin - f64| {dev:.3e} (tol {grad_tol(r, d32):.3e})")
        assert dev <= grad_tol(r, d32), name
    d32, dev = float(np.abs(y32[3] - ref[3]).max()), np.abs(got[3] - ref[3])
    _record(f"HOST_HEAD normalize {normalize} stats: d32 {d32:.3e}  |twin - f64| {dev.max():.3e} (tol {value_tol(ref[3], d32).min():.3e})")
    assert (dev <= value_tol(ref[3], d32)).all()


# ---- the plan ----
def test_ppo_query_accepts_and_refuses():
    from ev2gym_amd.engine import EngineError, ppo_query
    for net in ((162, 64, 64, 64, 64, 50), (63, 64, 64, 64, 64, 20), (192, 64, 64, 64, 64, 64), (1, 1, 1, 1, 1, 1)):
        info = ppo_query(*net)
        assert 0 < info["lds_bytes"] <= 160 * 1024 and info["grid_cap"] >= 1 and info["workspace_bytes"] > 0, (net, info)
        D, h1, h2, v1, v2, P = net
        assert info["n_params"] == h1 * D + h1 + h2 * h1 + h2 + v1 * D + v1 + v2 * v1 + v2 + P * h2 + P + v2 + 1 + P
    for net, word in (((193, 64, 64, 64, 64, 50), "d_in 193"), ((162, 64, 64, 64, 64, 65), "d_out 65"), ((162, 64, 0, 64, 64, 50), "h2 0"),
                      ((162, 64, 64, 64, 257, 50), "v2 257"), ((192, 128, 128, 128, 128, 64), "h1 128")):
        with pytest.raises(EngineError) as e:
            ppo_query(*net)
        assert e.value.code == -1 and word in str(e.value), (net, str(e.value))


# ---- Python-side refusals ----
def test_python_refusals():
    import torch
    from ev2gym_amd.onpolicy import GaussianActorCritic, RolloutBatch, init_ac_weights
    from ev2gym_amd.ppo import PPOLearner, check_batch
    for kw in (dict(batch_size=0), dict(n_epochs=0), dict(clip_range_vf=0.2), dict(target_kl=0.01), dict(lr=lambda f: 3e-4 * f), dict(use_masks=True),
               dict(ortho_init=True)):
        with pytest.raises(ValueError):
            PPOLearner(None, **kw)
    pol = GaussianActorCritic(init_ac_weights(6, 3, h=(4, 4), v=(4, 4)), np.zeros(3, np.float32))
    z = lambda *s: torch.zeros(s)  # noqa: E731
    good = dict(observations=z(5, 2, 6), actions=z(5, 2, 3), log_probs=z(5, 2), advantages=z(5, 2), returns=z(5, 2))
    assert check_batch(pol, RolloutBatch(**good)) == 10
    for bad in (dict(observations=z(5, 2, 7)), dict(actions=z(5, 2, 4)), dict(advantages=z(5, 3)), dict(log_probs=z(4, 2)), dict(returns=z(5, 1))):
        with pytest.raises(ValueError):
            check_batch(pol, RolloutBatch(**{**good, **bad}))
