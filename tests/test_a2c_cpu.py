"""The A2C learner's arithmetic without a GPU (ev2gym_amd/a2c.py, csrc/ev2g_ppo.h's host twins):

  * `a2c_update_numpy` (float64, analytic backprop) against torch float64 autograd of the loss written as SB3's A2C.train() writes it
    (`-(adv * log_prob).mean()`, `F.mse_loss`, `-torch.mean(entropy)`), to 1e-10 of each array's largest magnitude;
  * `rmsprop_numpy` + `clip_grad_norm_numpy` against torch.optim.RMSprop(alpha=0.99, eps=1e-5) and clip_grad_norm_ in float64, five steps, to 1e-12;
  * the host twins `ev2g_host_rmsprop` and `ev2g_host_a2c_head` (the device's element functions compiled for the host) against the float64
    references by the project's tolerance idiom (tests/test_ppo_cpu.py's docstring): 4 d32 + 4 * 2^-23 * s.  Every figure is printed before it
    is asserted, and appended to the file EV2G_PPO_RECORD names;
  * the Python-side refusals, and `ev2g_ppo_query` unchanged for the shapes tests/test_ppo_cpu.py lists.

A2C's head has no clip, so only the ReLU makes the gradient discontinuous: a ReLU case takes `make_case`'s seed rule (no float64
pre-activation with |z| < 1e-5).  The helpers are shared with tests/test_a2c_gpu.py."""
import numpy as np
import pytest

from tests.test_ppo_cpu import EPS32, _record, grad_tol, make_case, torch_params, value_tol


def a2c_reference(case, idx, **cfg):
    from ev2gym_amd.a2c import a2c_update_numpy
    return a2c_update_numpy(case["weights"], case["log_std"], case["obs"], case["actions"], case["advantages"], case["returns"], idx,
                            activation=case["activation"], **cfg)


def a2c_torch_loss(params, case, idx, dtype, vf_coef=0.5, ent_coef=0.0, normalize_advantage=False):
    """A2C.train()'s loss over the rows idx as SB3 writes it, in `dtype` on the CPU: (loss, the six statistics, the last two 0)."""
    import torch
    F = torch.nn.functional
    act = torch.tanh if case["activation"] == "tanh" else torch.relu
    t = lambda k: torch.tensor(np.asarray(case[k])[np.asarray(idx)], dtype=dtype)  # noqa: E731
    x, a, adv, ret = t("obs"), t("actions"), t("advantages"), t("returns")
    p = params
    mu = F.linear(act(F.linear(act(F.linear(x, p[0], p[1])), p[2], p[3])), p[8], p[9])
    v = F.linear(act(F.linear(act(F.linear(x, p[4], p[5])), p[6], p[7])), p[10], p[11]).flatten()
    dist = torch.distributions.Normal(mu, torch.ones_like(mu) * p[12].exp())
    lp, entropy = dist.log_prob(a).sum(dim=1), dist.entropy().sum(dim=1)
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pl = -(adv * lp).mean()
    vl = F.mse_loss(ret, v)
    el = -torch.mean(entropy)
    loss = pl + ent_coef * el + vf_coef * vl
    zero = torch.zeros((), dtype=dtype)
    return loss, [pl, vl, el, loss, zero, zero]


def a2c_torch_grads(case, idx, dtype, **cfg):
    """(the thirteen gradients, the six statistics) of one update by torch autograd in `dtype`, as float64 numpy arrays"""
    params = torch_params(case, dtype)
    loss, stats = a2c_torch_loss(params, case, idx, dtype, **cfg)
    loss.backward()
    return [p.grad.numpy().astype(np.float64) for p in params], np.array([float(s.detach()) for s in stats])


def a2c_torch_train(cases, index_sets, dtype, lr=7e-4, max_grad_norm=0.5, use_rms_prop=True, lrs=None, **cfg):
    """The loop a user has today: clip_grad_norm_ and torch.optim.RMSprop(alpha=0.99, eps=1e-5) (or Adam(eps=1e-5)), one update per
    (case, index set); the parameters start from cases[0]'s; lrs: the rate of each update, set in the optimiser's param group before it.
    (final parameters as float64 numpy, the statistics [n, 6], the gradient norms before clipping)"""
    import torch
    params = torch_params(cases[0], dtype)
    opt = torch.optim.RMSprop(params, lr=lr, alpha=0.99, eps=1e-5) if use_rms_prop else torch.optim.Adam(params, lr=lr, eps=1e-5)
    stats, norms = [], []
    for k, (case, idx) in enumerate(zip(cases, index_sets)):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        loss, st = a2c_torch_loss(params, case, idx, dtype, **cfg)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_grad_norm)))
        opt.step()
        stats.append([float(s.detach()) for s in st])
    return [p.detach().numpy().astype(np.float64) for p in params], np.array(stats), norms


# ---- a2c_update_numpy against torch float64 autograd ----
@pytest.mark.parametrize("B,normalize", [(2, True), (2, False), (37, True), (37, False), (1, False)])
@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_numpy_reference_matches_torch_float64_autograd(activation, ent_coef, B, normalize):
    import torch
    case = make_case(11, 5, h=(9, 6), v=(7, 10), activation=activation, n_rows=80)
    assert case["zmin"] >= 1e-5 or activation == "tanh"
    idx = np.random.default_rng(B).integers(0, 80, B)
    cfg = dict(vf_coef=0.5, ent_coef=ent_coef, normalize_advantage=normalize)
    grads, stats, _ = a2c_reference(case, idx, **cfg)
    tg, ts = a2c_torch_grads(case, idx, torch.float64, **cfg)
    for name, g, t in zip(range(13), grads, tg):
        assert g.shape == t.shape, name
        assert np.abs(g - t).max() <= 1e-10 * max(np.abs(t).max(), 1e-300), name
    assert (np.abs(stats - ts) <= 1e-10 * np.maximum(1.0, np.abs(ts))).all()
    assert stats[4] == 0.0 and stats[5] == 0.0


def test_numpy_reference_refuses_one_normalised_row():
    case = make_case(11, 5, h=(9, 6), v=(7, 10), n_rows=8)
    with pytest.raises(ValueError):
        a2c_reference(case, [3], normalize_advantage=True)


def test_rmsprop_and_clip_numpy_match_torch_float64():
    import torch
    from ev2gym_amd.a2c import clip_grad_norm_numpy, rmsprop_numpy
    rng = np.random.default_rng(3)
    shapes = [(6, 4), (6,), (3, 6), (3,)]
    theta = [rng.normal(size=s) for s in shapes]
    sq = [np.zeros(s) for s in shapes]
    params = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in theta]
    opt = torch.optim.RMSprop(params, lr=7e-4, alpha=0.99, eps=1e-5)
    for t in range(1, 6):
        g = [rng.normal(size=s) * (3.0 if t % 2 else 0.01) for s in shapes]   # the clip binds on odd steps only
        for p, gi in zip(params, g):
            p.grad = torch.tensor(gi)
        norm_t = float(torch.nn.utils.clip_grad_norm_(params, 0.5))
        opt.step()
        gc, norm = clip_grad_norm_numpy(g, 0.5)
        assert (norm > 0.5) == bool(t % 2) and abs(norm - norm_t) <= 1e-12 * norm_t
        for i in range(len(shapes)):
            theta[i], sq[i] = rmsprop_numpy(theta[i], sq[i], gc[i], lr=7e-4, alpha=0.99, eps=1e-5)
            ref = params[i].detach().numpy()
            assert np.abs(theta[i] - ref).max() <= 1e-12 * np.abs(ref).max(), (t, i)


# ---- the host twins ----
def test_host_rmsprop_against_rmsprop_numpy():
    import torch
    from ev2gym_amd.a2c import rmsprop_numpy
    from ev2gym_amd.engine import host_rmsprop
    rng = np.random.default_rng(5)
    n = 4099
    theta0 = rng.normal(0.0, 0.3, n).astype(np.float32)
    gs = [(rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32) for _ in range(5)]
    for g in gs:
        g[::41] = 0.0   # exact zeros: the step is 0 / (sqrt(sq) + eps), and sq only decays
    assert min(float(np.abs(g[g != 0]).min()) for g in gs) < 1e-5 and max(float(np.abs(g).max()) for g in gs) > 1.0
    th64, sq64 = theta0.astype(np.float64), np.zeros(n)
    th, sq = theta0.copy(), np.zeros(n, np.float32)
    p32 = torch.tensor(theta0, requires_grad=True)
    opt = torch.optim.RMSprop([p32], lr=7e-4, alpha=0.99, eps=1e-5)
    for t, g in enumerate(gs, start=1):
        th64, sq64 = rmsprop_numpy(th64, sq64, g, lr=7e-4, alpha=0.99, eps=1e-5)
        host_rmsprop(th, sq, g, lr=7e-4, alpha=0.99, eps=1e-5)
        p32.grad = torch.tensor(g)
        opt.step()
        d32 = float(np.abs(p32.detach().numpy() - th64).max())
        dev = np.abs(th - th64)
        _record(f"HOST_RMSPROP step {t}: d32 {d32:.3e}  |theta - f64| {dev.max():.3e} (tol {value_tol(th64, d32).min():.3e})")
        assert (dev <= value_tol(th64, d32)).all()
    assert np.abs(sq - sq64).max() <= 8 * EPS32 * np.abs(sq64).max()
    assert np.array_equal(th[::41], theta0[::41]) and not sq[::41].any()


@pytest.mark.parametrize("normalize,ent_coef", [(True, 0.0), (False, 0.01)])
def test_host_a2c_head_against_the_float64_head(normalize, ent_coef):
    import torch
    from ev2gym_amd.engine import host_a2c_head
    B, P = 97, 20
    rng = np.random.default_rng(9)
    mean = rng.normal(0.0, 0.5, (B, P)).astype(np.float32)
    value = rng.normal(0.0, 1.0, B).astype(np.float32)
    actions = (mean + rng.normal(0.0, 0.6, (B, P))).astype(np.float32)
    log_std = rng.uniform(-0.7, 0.0, P).astype(np.float32)
    adv, ret = rng.normal(0.0, 1.0, B).astype(np.float32), rng.normal(0.0, 1.0, B).astype(np.float32)

    def head(dtype):
        mu, v, ls = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (mean, value, log_std))
        dist = torch.distributions.Normal(mu, torch.ones_like(mu) * ls.exp())
        lp, ent = dist.log_prob(torch.tensor(actions, dtype=dtype)).sum(1), dist.entropy().sum(1)
        A = torch.tensor(adv, dtype=dtype)
        if normalize:
            A = (A - A.mean()) / (A.std() + 1e-8)
        pl = -(A * lp).mean()
        vl = torch.nn.functional.mse_loss(torch.tensor(ret, dtype=dtype), v)
        el = -ent.mean()
        loss = pl + ent_coef * el + 0.5 * vl
        loss.backward()
        return [mu.grad.numpy().astype(np.float64), v.grad.numpy().astype(np.float64), ls.grad.numpy().astype(np.float64),
                np.array([float(s.detach()) for s in (pl, vl, el, loss)] + [0.0, 0.0])]

    ref, y32 = head(torch.float64), head(torch.float32)
    got = host_a2c_head(mean, value, actions, log_std, adv, ret, vf_coef=0.5, ent_coef=ent_coef, normalize_advantage=normalize)
    for name, r, y, g in zip(("d_mean", "d_value", "d_log_std"), ref, y32, got):
        d32, dev = float(np.abs(y - r).max()), float(np.abs(g - r).max())
        _record(f"HOST_A2C_HEAD normalize {normalize} {name}: d32 {d32:.3e}  |twin - f64| {dev:.3e} (tol {grad_tol(r, d32):.3e})")
        assert dev <= grad_tol(r, d32), name
    d32, dev = float(np.abs(y32[3] - ref[3]).max()), np.abs(got[3] - ref[3])
    _record(f"HOST_A2C_HEAD normalize {normalize} stats: d32 {d32:.3e}  |twin - f64| {dev.max():.3e} (tol {value_tol(ref[3], d32).min():.3e})")
    assert (dev <= value_tol(ref[3], d32)).all()
    assert got[3][4] == 0.0 and got[3][5] == 0.0


def test_host_twins_refuse():
    from ev2gym_amd.engine import EngineError, host_a2c_head, host_rmsprop
    z = np.zeros((1, 3), np.float32)
    with pytest.raises(EngineError) as e:
        host_a2c_head(z, np.zeros(1), z, np.zeros(3), np.zeros(1), np.zeros(1), normalize_advantage=True)
    assert e.value.code == -1 and "normalize_advantage" in str(e.value)
    th, sq = np.zeros(4, np.float32), np.zeros(4, np.float32)
    for kw in (dict(alpha=1.0), dict(eps=0.0), dict(lr=float("nan"))):
        with pytest.raises(EngineError) as e:
            host_rmsprop(th, sq, np.ones(4, np.float32), **kw)
        assert e.value.code == -1


def test_config_mirror_matches_the_header():
    import os
    import re
    from conftest import ROOT
    from ev2gym_amd import _abi
    txt = open(os.path.join(ROOT, "include", "ev2g.h")).read()
    body = txt[txt.index("typedef struct ev2g_a2c_config {"):txt.index("} ev2g_a2c_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(kind, n) for kind, part in re.findall(r"(int32_t|double)\s+([^;]+);", body) for n in re.split(r"[,\s]+", part) if n]
    assert [n for _, n in fields] == [f[0] for f in _abi.A2cConfigC._fields_]
    assert [k for k, _ in fields] == ["double" if f[1] is _abi.C.c_double else "int32_t" for f in _abi.A2cConfigC._fields_]


# ---- the plan is PPO's, unchanged ----
def test_ppo_query_is_unchanged():
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
class _NoDevice:
    """A collector stand-in whose learner must be refused before anything touches a device."""
    policy = eng = None


def test_python_refusals():
    import torch
    from ev2gym_amd.a2c import A2CLearner
    from ev2gym_amd.onpolicy import GaussianActorCritic, RolloutBatch, init_ac_weights
    from ev2gym_amd.ppo import check_batch
    for kw in (dict(lr=lambda f: 7e-4 * f), dict(use_masks=True), dict(ortho_init=True), dict(policy_kwargs=dict(optimizer_class="RMSpropTFLike")),
               dict(RMSpropTFLike=True), dict(clip_range=0.2), dict(n_epochs=4), dict(batch_size=64), dict(target_kl=0.01), dict(n_steps=5)):
        with pytest.raises(ValueError):
            A2CLearner(_NoDevice(), **kw)
    pol = GaussianActorCritic(init_ac_weights(6, 3, h=(4, 4), v=(4, 4)), np.zeros(3, np.float32))
    z = lambda *s: torch.zeros(s)  # noqa: E731
    good = dict(observations=z(5, 2, 6), actions=z(5, 2, 3), log_probs=z(5, 2), advantages=z(5, 2), returns=z(5, 2), values=z(5, 2))
    assert check_batch(pol, RolloutBatch(**good), "A2CLearner.train") == 10
    learner = object.__new__(A2CLearner)   # train()'s checks come before its first device call
    learner.torch, learner.policy, learner.eng, learner.normalize_advantage = torch, pol, None, True
    for bad in (dict(observations=z(5, 2, 7)), dict(actions=z(5, 2, 4)), dict(advantages=z(5, 3)), dict(returns=z(5, 1)), dict(values=z(4, 2)),
                dict(use_masks=True), {k: v[:1, :1] for k, v in good.items()}):
        with pytest.raises(ValueError) as e:
            learner.train(RolloutBatch(**{**good, **bad}))
        assert "A2CLearner.train" in str(e.value)
