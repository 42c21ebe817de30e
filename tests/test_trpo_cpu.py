"""The TRPO learner's arithmetic without a GPU (ev2gym_amd/trpo.py, csrc/ev2g_trpo_host.h's plan and host twins):

  * `trpo_step_numpy` (float64, analytic gradient and analytic Fisher product) against a float64 torch restatement of sb3_contrib's
    TRPO.train(): KL from torch.distributions, H v from two autograd.grad calls, Python conjugate gradient and line search.  g, one H v for a
    random v to 1e-9 of the array's largest magnitude; x, beta, every try's (KL, J) and the final parameters to 1e-7 after five iterations,
    and x after the default fifteen to the bound both solutions' residuals give;
  * the host twins `ev2g_host_trpo_cg_step` and `ev2g_host_trpo_rows` against the numpy statement;
  * the config mirror against the header, `ev2g_trpo_query` over tests/learner_cases.py's networks and PPO's refusals, with
    `ev2g_ppo_query`'s own figures unchanged, and the Python-side refusals.

The helpers are shared with tests/test_trpo_gpu.py."""
import numpy as np
import pytest

from tests.test_ppo_cpu import make_case, torch_params

ACTOR = (12, 0, 1, 2, 3, 8, 9)   # log_std, pi_W1, pi_b1, pi_W2, pi_b2, action_W, action_b in the thirteen arrays' order


def trpo_reference(case, idx, **cfg):
    from ev2gym_amd.trpo import trpo_step_numpy
    return trpo_step_numpy(case["weights"], case["log_std"], case["obs"], case["actions"], case["old_log_prob"], case["advantages"], idx,
                           activation=case["activation"], **cfg)


class TorchTrpo:
    """sb3_contrib's TRPO.train() policy step restated in torch on the CPU in `dtype`: what a torch user runs today."""

    def __init__(self, case, idx, dtype, normalize_advantage=True, params=None):
        import torch
        self.torch, self.dtype = torch, dtype
        self.params = torch_params(case, dtype) if params is None else params
        self.actor = [self.params[i] for i in ACTOR]
        self.act = torch.tanh if case["activation"] == "tanh" else torch.relu
        t = lambda k: torch.tensor(np.asarray(case[k])[np.asarray(idx)], dtype=dtype)  # noqa: E731
        self.x, self.a, self.old, adv = t("obs"), t("actions"), t("old_log_prob"), t("advantages")
        if normalize_advantage and len(adv) > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        self.adv = adv

    def dist(self):
        torch, p, F = self.torch, self.params, self.torch.nn.functional
        mu = F.linear(self.act(F.linear(self.act(F.linear(self.x, p[0], p[1])), p[2], p[3])), p[8], p[9])
        return torch.distributions.Normal(mu, torch.ones_like(mu) * p[12].exp())

    def objective(self, dist):
        return (self.adv * self.torch.exp(dist.log_prob(self.a).sum(dim=1) - self.old)).mean()

    def kl(self, dist, old):
        return self.torch.distributions.kl_divergence(dist, old).sum(dim=1).mean()

    def flat(self, arrays):
        return np.concatenate([a.detach().numpy().astype(np.float64).ravel() for a in arrays])

    def split(self, v):
        out, o = [], 0
        for p in self.actor:
            out.append(self.torch.tensor(np.asarray(v[o:o + p.numel()]), dtype=self.dtype).reshape(p.shape))
            o += p.numel()
        return out

    def start(self):
        torch = self.torch
        d = self.dist()
        self.old_dist = torch.distributions.Normal(d.loc.detach(), d.scale.detach())
        J = self.objective(d)
        self.g = self.flat(torch.autograd.grad(J, self.actor, retain_graph=True))
        self.grad_kl = torch.autograd.grad(self.kl(d, self.old_dist), self.actor, create_graph=True)
        self.J0 = float(J.detach())
        return self.g

    def hvp(self, v, damping):
        torch = self.torch
        vs = self.split(v)
        jvp = sum((gk * vk).sum() for gk, vk in zip(self.grad_kl, vs))
        hv = torch.autograd.grad(jvp, self.actor, retain_graph=True)
        return self.flat(hv) + damping * self.flat(vs)

    def step(self, target_kl=0.01, cg_damping=0.1, cg_max_steps=15, line_search_shrinking_factor=0.8, line_search_max_iter=10):
        from ev2gym_amd.trpo import cg_numpy
        torch = self.torch
        g = self.start()
        cast = lambda v: self.flat(self.split(v))  # noqa: E731  (the vector in `dtype`, as the torch loop keeps it)
        fvp = lambda v: self.hvp(v, cg_damping)  # noqa: E731
        x, iters = cg_numpy(fvp, g, cg_max_steps)
        x = cast(x)
        xHx = float(x @ fvp(x))
        out = dict(g=g, x=x, objective_before=self.J0, xHx=xHx, cg_iterations=iters, tries=[], accepted=False, kl=0.0, objective_after=0.0,
                   failed=not (np.isfinite(xHx) and xHx > 0.0), beta=0.0)
        theta0 = [p.detach().clone() for p in self.actor]
        if not out["failed"]:
            beta = out["beta"] = float(np.sqrt(2.0 * target_kl / xHx))
            c = 1.0
            with torch.no_grad():
                for _ in range(line_search_max_iter):
                    for p, p0, dx in zip(self.actor, theta0, self.split(x)):
                        p.copy_(p0 + c * beta * dx)
                    d = self.dist()
                    KL, J = float(self.kl(d, self.old_dist)), float(self.objective(d))
                    out["tries"].append((KL, J))
                    out["kl"], out["objective_after"] = KL, J
                    if KL < target_kl and J > self.J0:
                        out["accepted"] = True
                        break
                    c *= line_search_shrinking_factor
                if not out["accepted"]:
                    for p, p0 in zip(self.actor, theta0):
                        p.copy_(p0)
        out["line_search_tries"] = len(out["tries"])
        out["params"] = [p.detach().numpy().astype(np.float64) for p in self.actor]
        return out


def decisions(step, target_kl):
    """The line search's verdict per try, and the margins of the closest one: (list of bools, min |KL - target| / target, min |J - J0| / max(1, |J0|))"""
    J0 = step["objective_before"]
    oks = [KL < target_kl and J > J0 for KL, J in step["tries"]]
    mk = min((abs(KL - target_kl) / target_kl for KL, _ in step["tries"]), default=np.inf)
    mj = min((abs(J - J0) / max(1.0, abs(J0)) for _, J in step["tries"]), default=np.inf)
    return oks, mk, mj


def _close(a, b, rel, name):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, name
    assert np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-300), (name, float(np.abs(a - b).max()), float(np.abs(b).max()))


# ---- trpo_step_numpy against the torch float64 restatement ----
@pytest.mark.parametrize("B", [1, 33, 97])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_numpy_reference_matches_the_torch_float64_restatement(activation, B):
    import torch
    from ev2gym_amd.trpo import trpo_fvp_numpy
    case = make_case(11, 5, h=(9, 6), v=(7, 10), activation=activation, n_rows=120)
    idx = np.random.default_rng(B).integers(0, 120, B)
    # Five iterations pin the algebra: rounding differences between the two products (1e-16) have not grown yet.  At the default fifteen the
    # solve is near convergence, where conjugate gradient amplifies them (measured: 1e-15 after 6 iterations, 1e-12 after 10, 1e-6 after 13), so x
    # is held to what both solutions must satisfy: |x1 - x2| <= (|H x1 - g| + |H x2 - g|) / lambda_min(H), lambda_min >= cg_damping.
    full, tfull = trpo_reference(case, idx), TorchTrpo(case, idx, torch.float64)
    tsf = tfull.step()
    chk = TorchTrpo(case, idx, torch.float64)   # (a step moves its own parameters: the products at theta0 come from a fresh one)
    chk.start()
    res = sum(np.linalg.norm(chk.hvp(s["x"], 0.1) - s["g"]) for s in (full, tsf))
    assert np.abs(full["x"] - tsf["x"]).max() <= res / 0.1 + 1e-9 * np.abs(tsf["x"]).max()
    # (the iteration at which r . r crosses 1e-10 is not reproducible either: 13 here against 15 there for the same solution)
    assert full["accepted"] == tsf["accepted"] and full["line_search_tries"] == tsf["line_search_tries"]
    ref = trpo_reference(case, idx, cg_max_steps=5)
    tt = TorchTrpo(case, idx, torch.float64)
    ts = tt.step(cg_max_steps=5)
    _close(ref["g"], ts["g"], 1e-9, "g")
    v = np.random.default_rng(B + 1).normal(size=ref["g"].size)
    for damping in (0.0, 0.1):
        _close(trpo_fvp_numpy(case["weights"], case["log_std"], case["obs"], idx, v, activation=activation, cg_damping=damping), chk.hvp(v, damping),
               1e-9, f"Hv damping {damping}")
    _close(ref["x"], ts["x"], 1e-7, "x")
    assert ref["cg_iterations"] == ts["cg_iterations"] and ref["line_search_tries"] == ts["line_search_tries"] >= 1
    assert ref["accepted"] == ts["accepted"] and not ref["failed"]
    assert abs(ref["beta"] - ts["beta"]) <= 1e-7 * ts["beta"] and abs(ref["objective_before"] - ts["objective_before"]) <= 1e-12
    for (k1, j1), (k2, j2) in zip(ref["tries"], ts["tries"]):
        assert abs(k1 - k2) <= 1e-7 * max(1.0, abs(k2)) and abs(j1 - j2) <= 1e-7 * max(1.0, abs(j2))
    for name, a, b in zip(range(7), ref["params"], ts["params"]):
        _close(a, b, 1e-7, name)


def test_numpy_reference_branches():
    """A rejected first try, a failed search that leaves theta0, one conjugate-gradient step, and the vanishing-gradient exit."""
    case = make_case(11, 5, h=(9, 6), v=(7, 10), n_rows=120)
    idx = np.arange(97)
    big = trpo_reference(case, idx, target_kl=16.0)
    assert big["line_search_tries"] >= 2 and big["accepted"]
    fail = trpo_reference(case, idx, target_kl=16.0, line_search_max_iter=1)
    assert not fail["accepted"] and not fail["failed"] and fail["line_search_tries"] == 1
    from ev2gym_amd.trpo import actor_arrays
    for a, b in zip(fail["params"], actor_arrays(case["weights"], case["log_std"])):
        assert np.array_equal(a, b)
    assert trpo_reference(case, idx, cg_max_steps=1)["cg_iterations"] == 1
    flat = dict(case, advantages=case["advantages"] * 1e-9)
    none = trpo_reference(flat, idx, normalize_advantage=False)
    assert none["cg_iterations"] == 0 and none["failed"] and none["line_search_tries"] == 0 and not none["x"].any()


# ---- the host twins ----
def test_host_cg_step_against_cg_numpy():
    from ev2gym_amd.engine import host_trpo_cg_step
    rng = np.random.default_rng(4)
    n = 301
    M = rng.normal(size=(n, n))
    H = M @ M.T / n + 0.1 * np.eye(n)
    g = rng.normal(size=n)
    from ev2gym_amd.trpo import cg_numpy
    f32 = lambda v: v.astype(np.float32).astype(np.float64)  # noqa: E731
    for steps in (1, 3, 15):
        # the twin keeps p float32-representable, as the device does (its product reads p's float32 image): the same algebra written out here
        xm, rm, pm, rhom = np.zeros(n), g.copy(), f32(g), float(g @ g)
        x, r, p, rho = np.zeros(n), g.copy(), f32(g), float(g @ g)
        done, k = False, 0
        while not done:
            Hp = H @ pm
            alpha = rhom / float(pm @ Hp)
            xm = xm + alpha * pm
            if k < steps - 1:
                rm = rm - alpha * Hp
                new = float(rm @ rm)
                pm, rhom = f32(rm + (new / rhom) * pm), new
            rho, done = host_trpo_cg_step(x, r, p, H @ p, rho, last=(k == steps - 1))
            k += 1
        assert k == steps
        assert np.abs(x - xm).max() <= 1e-12 * np.abs(xm).max() and np.array_equal(p, f32(p))
        # ... and it is conjugate gradient: the rounding of p costs no more than float32's own resolution against the unrounded solve
        want, iters = cg_numpy(lambda v: H @ v, g, steps)
        assert iters == steps and np.abs(x - want).max() <= 1e-5 * np.abs(want).max()
    # the 1e-10 exit: an exact solve in one step
    x, r, p = np.zeros(4), np.array([1.0, 0, 0, 0]), np.array([1.0, 0, 0, 0])
    rho, done = host_trpo_cg_step(x, r, p, 2.0 * p, 1.0, last=False)
    assert done and rho < 1e-10 and np.array_equal(x, [0.5, 0, 0, 0])


@pytest.mark.parametrize("normalize", [True, False])
def test_host_rows_against_the_float64_rows(normalize):
    from ev2gym_amd.engine import host_trpo_rows
    B, P = 97, 20
    rng = np.random.default_rng(9)
    mean = rng.normal(0.0, 0.5, (B, P)).astype(np.float32)
    mean0 = (mean + rng.normal(0.0, 0.05, (B, P))).astype(np.float32)
    actions = (mean + rng.normal(0.0, 0.6, (B, P))).astype(np.float32)
    ls = rng.uniform(-0.7, 0.0, P).astype(np.float32)
    ls0 = (ls + rng.normal(0.0, 0.02, P)).astype(np.float32)
    adv = rng.normal(0.0, 1.0, B).astype(np.float32)
    m, m0, a, l, l0, A = (v.astype(np.float64) for v in (mean, mean0, actions, ls, ls0, adv))
    lp = (-(a - m) ** 2 * 0.5 * np.exp(-2 * l) - l - 0.5 * np.log(2 * np.pi)).sum(1)
    old = (lp + rng.normal(0.0, 0.3, B)).astype(np.float32)
    if normalize:
        A = (A - A.mean()) / (A.std(ddof=1) + 1e-8)
    j_ref = A * np.exp(lp - old.astype(np.float64))
    kl_ref = (l0 - l + (np.exp(2 * l) + (m - m0) ** 2) / (2 * np.exp(2 * l0)) - 0.5).sum(1)
    j, kl = host_trpo_rows(mean, mean0, actions, ls, ls0, old, adv, normalize_advantage=normalize)
    # float64 arithmetic on float32 operands; the normalised advantage is rounded to float32 once, as the device rounds it
    assert np.abs(j - j_ref).max() <= 4 * 2.0 ** -23 * np.abs(j_ref).max()
    assert np.abs(kl - kl_ref).max() <= 1e-12 * np.abs(kl_ref).max()


def test_host_twins_refuse():
    from ev2gym_amd.engine import EngineError, host_trpo_rows
    z = np.zeros((0, 3), np.float32)
    with pytest.raises(EngineError) as e:
        host_trpo_rows(z, z, z, np.zeros(3), np.zeros(3), np.zeros(0), np.zeros(0))
    assert e.value.code == -1


def test_config_mirror_matches_the_header():
    import os
    import re
    from conftest import ROOT
    from ev2gym_amd import _abi
    txt = open(os.path.join(ROOT, "include", "ev2g.h")).read()
    for cname, mirror in (("ev2g_trpo_config", _abi.TrpoConfigC), ("ev2g_trpo_info", _abi.TrpoInfoC), ("ev2g_trpo_report", _abi.TrpoReportC)):
        body = txt[txt.index("typedef struct %s {" % cname):txt.index("} %s;" % cname)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [(kind, n) for kind, part in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body) for n in re.split(r"[,\s]+", part) if n]
        assert [n for _, n in fields] == [f[0] for f in mirror._fields_], cname
        ctype = {_abi.C.c_double: "double", _abi.C.c_int32: "int32_t", _abi.C.c_int64: "int64_t"}
        assert [k for k, _ in fields] == [ctype[f[1]] for f in mirror._fields_], cname


# ---- the plan: everything PPO's accepts, never more LDS, PPO's own figures unchanged ----
def test_trpo_query():
    from ev2gym_amd.engine import EngineError, ppo_query, trpo_query
    from tests.learner_cases import LEARNER_NETS, net_shape
    nets = [net_shape(tag) for tag in LEARNER_NETS] + [(162, 64, 64, 64, 64, 50), (63, 64, 64, 64, 64, 20), (192, 64, 64, 64, 64, 64), (1, 1, 1, 1, 1, 1),
                                                        (63, 33, 17, 40, 64, 20)]
    for net in nets:
        info, ppo = trpo_query(*net), ppo_query(*net)
        D, h1, h2, v1, v2, P = net
        assert 0 < info["lds_bytes"] <= ppo["lds_bytes"] <= 160 * 1024, (net, info)
        assert info["grid_cap"] == ppo["grid_cap"] and info["n_params"] == ppo["n_params"] and info["workspace_bytes"] > ppo["workspace_bytes"]
        assert info["n_actor"] == P + h1 * D + h1 + h2 * h1 + h2 + P * h2 + P
    for tag, row in LEARNER_NETS.items():
        assert ppo_query(*net_shape(tag))["lds_bytes"] == row[5], tag   # (PPO's plan is what it was)
    for net, word in (((193, 64, 64, 64, 64, 50), "d_in 193"), ((162, 64, 64, 64, 64, 65), "d_out 65"), ((162, 64, 0, 64, 64, 50), "h2 0"),
                      ((162, 64, 64, 64, 257, 50), "v2 257"), ((192, 128, 128, 128, 128, 64), "h1 128")):
        for query in (ppo_query, trpo_query):
            with pytest.raises(EngineError) as e:
                query(*net)
            assert e.value.code == -1 and word in str(e.value), (net, str(e.value))


# ---- Python-side refusals ----
class _NoDevice:
    """A collector stand-in whose learner must be refused before anything touches a device."""
    policy = eng = None


def test_python_refusals():
    import torch
    from ev2gym_amd.onpolicy import GaussianActorCritic, RolloutBatch, init_ac_weights
    from ev2gym_amd.trpo import TRPOLearner
    for kw in (dict(learning_rate=lambda f: 1e-3 * f), dict(use_sde=True), dict(use_masks=True), dict(policy_kwargs=dict(share_features_extractor=True)),
               dict(clip_range=0.2), dict(n_epochs=4), dict(n_steps=2048), dict(batch_size=0), dict(sub_sampling_factor=0), dict(cg_max_steps=0),
               dict(line_search_max_iter=0), dict(n_critic_updates=-1)):
        with pytest.raises(ValueError) as e:
            TRPOLearner(_NoDevice(), **kw)
        assert "TRPOLearner" in str(e.value)
    pol = GaussianActorCritic(init_ac_weights(6, 3, h=(4, 4), v=(4, 4)), np.zeros(3, np.float32))
    z = lambda *s: torch.zeros(s)  # noqa: E731
    good = dict(observations=z(5, 2, 6), actions=z(5, 2, 3), log_probs=z(5, 2), advantages=z(5, 2), returns=z(5, 2), values=z(5, 2))
    learner = object.__new__(TRPOLearner)   # train()'s checks come before its first device call
    learner.torch, learner.policy, learner.eng = torch, pol, None
    for bad in (dict(observations=z(5, 2, 7)), dict(actions=z(5, 2, 4)), dict(advantages=z(5, 3)), dict(returns=z(5, 1)), dict(use_masks=True)):
        with pytest.raises(ValueError) as e:
            learner.train(RolloutBatch(**{**good, **bad}))
        assert "TRPOLearner.train" in str(e.value)
