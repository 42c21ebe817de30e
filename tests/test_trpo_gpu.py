"""The TRPO learner on the device (csrc/ev2g_trpo.h; ev2g_trpo_*; ev2gym_amd/trpo.py): the objective's gradient and J(theta0), the
Fisher-vector product, the whole policy step at 1, 3 and 15 conjugate-gradient iterations, every branch of the line search, the critic's
gradient and Adam steps, bit-for-bit determinism, the repacked weight images against a fresh policy object, TRPOLearner.train() / learn() end to
end behind a collector, and every refusal through the ABI.

Tolerance (the idiom of tests/test_ppo_gpu.py): reference = float64 (`trpo_step_numpy`, or the torch float64 loop); d32 = the largest deviation
from it of the same computation in torch-CPU float32 (tests/test_trpo_cpu.py's TorchTrpo: double backward, Python conjugate gradient and line
search); the device gets 4 d32 + 4 * 2^-23 * s with s = max(1, |y|) for parameters and scalars and the array's largest reference magnitude
for gradients, products and x.  Every d32 and every device deviation is printed before it is asserted, and appended to the file
EV2G_PPO_RECORD names.

The line search is discontinuous in its two conditions, and the conjugate-gradient exit in r . r, so every step case is first checked ON THE
REFERENCE to sit away from them: every try keeps |KL - target_kl| >= 1e-3 target_kl and |J - J(theta0)| >= 1e-4 max(1, |J(theta0)|), torch
float32 takes the same decisions, and no r . r the exit tests lies within a factor 100 of 1e-10."""
import numpy as np
import pytest

from tests.learner_cases import LEARNER_NETS, N_ROWS, NAMES, SHAPES, _index_sets, _shape, engines  # noqa: F401 (engines: the fixture)
from tests.test_onpolicy_gpu import _bits, _gen_engine, _up
from tests.test_ppo_cpu import EPS32, _record, grad_tol, make_case, torch_params, value_tol
from tests.test_trpo_cpu import ACTOR, TorchTrpo, decisions, trpo_reference

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
VALUE = (4, 5, 6, 7, 10, 11)   # the six value arrays among the thirteen


def _flat(arrays13):
    return np.concatenate([np.asarray(arrays13[i], np.float64).ravel() for i in ACTOR])


class _Trpo:
    """A case's rows, a policy object and a TRPO learner on an engine."""

    def __init__(self, eng, case, lo=-1.0, **cfg):
        from ev2gym_amd.engine import trpo_query
        from ev2gym_amd.onpolicy import GaussianActorCritic
        self.eng, self.case = eng, case
        self.pol = GaussianActorCritic(case["weights"], case["log_std"], activation=case["activation"], lo=lo, seed=5).attach(eng)
        self.trpo = eng.trpo_create(self.pol.ac, **cfg)
        self.n_actor = trpo_query(*_shape(case))["n_actor"]
        self.obs, self.actions, self.old, self.adv, self.ret = (_up(eng, case[k]) for k in ("obs", "actions", "old_log_prob", "advantages", "returns"))
        self.obj, self.vl = eng.empty((1,), np.float64), eng.empty((1,), np.float32)
        self.v, self.hv = eng.empty((self.n_actor,), np.float32), eng.empty((self.n_actor,), np.float32)

    def grad(self, idx):
        ix = _up(self.eng, np.asarray(idx, np.int32))
        self.eng.trpo_grad(self.trpo, self.obs, self.actions, self.old, self.adv, ix, len(idx), self.obj)
        g = self.eng.ppo_get_grads(self.trpo, _shape(self.case))
        J = float(self.obj.to_host()[0])
        ix.free()
        return g, J

    def fvp(self, idx, v):
        ix = _up(self.eng, np.asarray(idx, np.int32))
        self.v.upload(np.ascontiguousarray(v, np.float32))
        self.eng.trpo_fvp(self.trpo, self.obs, ix, len(idx), self.v, self.hv)
        out = self.hv.to_host().astype(np.float64)
        ix.free()
        return out

    def step(self, idx):
        ix = _up(self.eng, np.asarray(idx, np.int32))
        self.eng.trpo_policy_step(self.trpo, self.obs, self.actions, self.old, self.adv, ix, len(idx))
        rep = self.eng.trpo_get_report(self.trpo)
        x, g = self.eng.trpo_get_direction(self.trpo, self.n_actor)
        ix.free()
        return rep, x, g

    def critic(self, idx):
        ix = _up(self.eng, np.asarray(idx, np.int32))
        self.eng.trpo_critic_minibatch(self.trpo, self.obs, self.ret, ix, len(idx), self.vl)
        out = float(self.vl.to_host()[0])
        ix.free()
        return out

    def weights(self):
        w, ls = self.eng.ac_get_weights(self.pol.ac, _shape(self.case))
        return w + [ls]

    def close(self):
        self.pol.close()   # (the learner goes with its policy)
        for b in (self.obs, self.actions, self.old, self.adv, self.ret, self.obj, self.vl, self.v, self.hv):
            b.free()


def _vec(tag, name, got, ref, y32):
    d32, dev = float(np.abs(y32 - ref).max()), float(np.abs(got - ref).max())
    tol = grad_tol(ref, d32)
    _record(f"TRPO {tag} {name}: d32 {d32:.3e}  |device - f64| {dev:.3e}  tol {tol:.3e}  max|ref| {np.abs(ref).max():.3e}")
    return bool(np.isfinite(got).all() and dev <= tol)


def _val(tag, name, got, ref, y32):
    got, ref, y32 = (np.asarray(a, np.float64) for a in (got, ref, y32))
    d32, dev, tol = float(np.abs(y32 - ref).max()), np.abs(got - ref), value_tol(ref, float(np.abs(y32 - ref).max()))
    _record(f"TRPO {tag} {name}: d32 {d32:.3e}  |device - f64| {float(dev.max()):.3e}  tol {float(np.min(tol)):.3e}")
    return bool(np.isfinite(got).all() and (dev <= tol).all())


NET_CASES = [("pst-tanh", "pst", 63, (64, 64), (64, 64), 20, "tanh"), ("ppl-tanh", "ppl", 162, (64, 64), (64, 64), 50, "tanh"),
             ("pst-relu", "pst", 63, (64, 64), (64, 64), 20, "relu"), ("ppl-relu", "ppl", 162, (64, 64), (64, 64), 50, "relu"),
             ("pst-odd", "pst", 63, (33, 17), (40, 64), 20, "tanh")]
NET_CASES += [(f"{tag}-{a}", "pst", d_in, h, v, d_out, a) for tag, (d_in, h, v, d_out, acts, _) in LEARNER_NETS.items() for a in acts]


@pytest.mark.parametrize("tag,kind,D,h,v,P,activation", NET_CASES, ids=[c[0] for c in NET_CASES])
def test_gradient_objective_and_fisher_products(engines, tag, kind, D, h, v, P, activation):
    """g and J(theta0) over every row set, the six value arrays of the gradient untouched; H v for v = g, a random v and a v in log_std only, at
    cg_damping 0.1 and 0; one normalised row is skipped silently, as PPO does."""
    import torch
    from ev2gym_amd.engine import trpo_query
    from ev2gym_amd.trpo import trpo_fvp_numpy
    eng = engines[kind]
    n_rows = N_ROWS[activation]
    case = make_case(D, P, h=h, v=v, activation=activation, n_rows=n_rows)
    if activation == "relu":
        assert case["zmin"] >= 1e-5
    cap = trpo_query(*_shape(case))["grid_cap"]
    sets = _index_sets(cap, n_rows)
    ok = True
    for damping in (0.1, 0.0):
        dev = _Trpo(eng, case, cg_damping=damping)
        try:
            for idx in sets:
                B = len(idx)
                ref = trpo_reference(case, idx, cg_max_steps=1, line_search_max_iter=1)
                tt = TorchTrpo(case, idx, torch.float32)
                g32 = tt.start()
                if damping == 0.1:
                    before = dev.eng.ppo_get_grads(dev.trpo, _shape(case))
                    got, J = dev.grad(idx)
                    ok &= _vec(f"GRAD {tag} B {B}", "g", _flat(got), ref["g"], g32)
                    ok &= _val(f"GRAD {tag} B {B}", "J(theta0)", J, ref["objective_before"], tt.J0)
                    for i in VALUE:
                        assert np.array_equal(_bits(got[i]), _bits(before[i])), NAMES[i]
                rng = np.random.default_rng(B)
                only_ls = np.zeros(ref["g"].size)
                only_ls[:P] = rng.normal(size=P)
                for name, vec in (("v = g", ref["g"]), ("random v", rng.normal(size=ref["g"].size)), ("v in log_std", only_ls)):
                    v32 = vec.astype(np.float32).astype(np.float64)   # (what the device is given)
                    want = trpo_fvp_numpy(case["weights"], case["log_std"], case["obs"], idx, v32, activation=activation, cg_damping=damping)
                    hv = dev.fvp(idx, v32)
                    ok &= _vec(f"FVP {tag} B {B} damping {damping}", name, hv, want, tt.hvp(v32, damping))
                    if name == "v in log_std":   # the block is (2 + damping) v to float32 rounding, the rest is damping v = 0
                        assert np.abs(hv[:P] - (2.0 + damping) * v32[:P]).max() <= 2 * EPS32 * np.abs((2.0 + damping) * v32[:P]).max()
                        assert not hv[P:].any()
        finally:
            dev.close()
    assert ok


def _margins(tag, ref, y32, target_kl):
    """The reference sits away from every discontinuity, and torch float32 decides as it does."""
    oks, mk, mj = decisions(ref, target_kl)
    _record(f"TRPO MARGIN {tag}: tries {ref['tries']}  min |KL - target| / target {mk:.3e}  min |J - J0| / max(1, |J0|) {mj:.3e}  "
            f"min r.r {min(ref['rho_history']):.3e}")
    assert mk >= 1e-3 and mj >= 1e-4
    assert decisions(y32, target_kl)[0] == oks and y32["cg_iterations"] == ref["cg_iterations"] and y32["accepted"] == ref["accepted"]
    assert all(r >= 1e-8 or r <= 1e-12 for r in ref["rho_history"])


def _compare_step(tag, dev, case, idx, cfg):
    import torch
    target_kl = cfg.get("target_kl", 0.01)
    ref = trpo_reference(case, idx, **cfg)
    y32 = TorchTrpo(case, idx, torch.float32).step(**cfg)
    _margins(tag, ref, y32, target_kl)
    before = dev.weights()
    rep, x, g = dev.step(idx)
    after = dev.weights()
    assert rep["cg_iterations"] == ref["cg_iterations"] and rep["line_search_tries"] == ref["line_search_tries"], (rep, ref["tries"])
    assert bool(rep["accepted"]) == ref["accepted"] and bool(rep["failed"]) == ref["failed"]
    ok = _vec(tag, "g", g, ref["g"], y32["g"]) & _vec(tag, "x", x, ref["x"], y32["x"])
    ok &= _val(tag, "beta", rep["beta"], ref["beta"], y32["beta"]) & _val(tag, "x.Hx", rep["xHx"], ref["xHx"], y32["xHx"])
    ok &= _val(tag, "J(theta0)", rep["objective_before"], ref["objective_before"], y32["objective_before"])
    if ref["tries"]:
        ok &= _val(tag, "KL of the last try", rep["kl"], ref["kl"], y32["kl"]) & _val(tag, "J of the last try", rep["objective_after"], ref["objective_after"], y32["objective_after"])
        assert abs(rep["c"] - ref["c"]) <= 1e-15
    for k, i in enumerate(ACTOR):
        ok &= _val(tag, NAMES[i], after[i], ref["params"][k], y32["params"][k])
    for i in VALUE:
        assert np.array_equal(_bits(after[i]), _bits(before[i])), NAMES[i]
    return ok, ref, before, after


@pytest.mark.parametrize("cg_max_steps", [1, 3, 15])
def test_policy_step_matches_the_float64_reference(engines, cg_max_steps):
    from ev2gym_amd.engine import trpo_query
    eng, (D, P) = engines["pst"], SHAPES["pst"]
    case = make_case(D, P, n_rows=600)
    cap = trpo_query(*_shape(case))["grid_cap"]
    sets = _index_sets(cap, 600)
    ok = True
    for idx in (sets[3], sets[4], sets[5]):   # 33 rows, 97 with duplicates, every workgroup looping
        dev = _Trpo(eng, case, cg_max_steps=cg_max_steps)
        try:
            good, ref, _, _ = _compare_step(f"STEP cg_max_steps {cg_max_steps} B {len(idx)}", dev, case, idx, dict(cg_max_steps=cg_max_steps))
            ok &= good
            assert ref["accepted"]
        finally:
            dev.close()
    assert ok


def test_a_vanishing_gradient_leaves_the_parameters(engines):
    """rho < 1e-10 before the first iteration: no iteration, no try, the step marked failed, every array bit-identical."""
    import torch
    eng, (D, P) = engines["pst"], SHAPES["pst"]
    case = dict(make_case(D, P, n_rows=600))
    case["advantages"] = (case["advantages"] * 1e-9).astype(np.float32)
    idx = np.random.default_rng(12).choice(600, 97)
    ref = trpo_reference(case, idx, normalize_advantage=False)
    assert ref["rho_history"][0] < 1e-12 and ref["cg_iterations"] == 0 and ref["failed"]
    dev = _Trpo(eng, case, normalize_advantage=False)
    try:
        before = dev.weights()
        rep, x, g = dev.step(idx)
        _record(f"TRPO EARLY EXIT: rho f64 {ref['rho_history'][0]:.3e}  report {rep}")
        assert rep["cg_iterations"] == 0 and rep["line_search_tries"] == 0 and rep["failed"] and not rep["accepted"] and not x.any()
        assert _vec("EARLY EXIT", "g", g, ref["g"], TorchTrpo(case, idx, torch.float32, normalize_advantage=False).start())
        for a, b in zip(dev.weights(), before):
            assert np.array_equal(_bits(a), _bits(b))
    finally:
        dev.close()


LS_CASES = [("first-try", 97, {}, 1, True), ("rejected-on-both", 97, dict(target_kl=16.0), 2, True),
            ("rejected-on-kl", 33, dict(target_kl=0.5, cg_damping=1e-3), 2, True),
            ("failed-16", 97, dict(target_kl=16.0, line_search_max_iter=1), 1, False),
            ("failed-0.5", 33, dict(target_kl=0.5, cg_damping=1e-3, line_search_max_iter=1), 1, False)]


@pytest.mark.parametrize("tag,B,cfg,tries,accepted", LS_CASES, ids=[c[0] for c in LS_CASES])
def test_line_search_branches(engines, tag, B, cfg, tries, accepted):
    from ev2gym_amd.onpolicy import GaussianActorCritic
    eng, (D, P) = engines["pst"], SHAPES["pst"]
    case = make_case(D, P, n_rows=600)
    idx = np.random.default_rng(12).choice(600, B)
    dev = _Trpo(eng, case, **cfg)
    twin = None
    try:
        ok, ref, before, after = _compare_step(f"LINE SEARCH {tag}", dev, case, idx, cfg)
        assert ok and ref["line_search_tries"] == tries and ref["accepted"] == accepted
        if tag == "rejected-on-both":
            assert ref["tries"][0][0] > 16.0 and ref["tries"][0][1] < ref["objective_before"]
        if tag == "rejected-on-kl":
            assert ref["tries"][0][0] > 0.5 and ref["tries"][0][1] > ref["objective_before"]
        if not accepted:   # masters, images and transposed images as before: bit-identical outputs, and a second step decides the same
            for a, b in zip(after, before):
                assert np.array_equal(_bits(a), _bits(b))
            twin = GaussianActorCritic(case["weights"], case["log_std"], activation="tanh", lo=-1.0, seed=5).attach(eng)
            dx = _up(eng, case["obs"][:37])
            out = [eng.empty((37, P), np.float32) for _ in range(2)]
            for ac, m in zip((dev.pol.ac, twin.ac), out):
                eng.ac_forward(ac, dx, 37, mean=m)
            eng.synchronize()
            assert np.array_equal(_bits(out[0].to_host()), _bits(out[1].to_host()))
            rep1, x1, _ = dev.step(idx)   # (the transposed images feed the backward passes: the same x to the bit)
            fresh = _Trpo(eng, case, **cfg)
            try:
                rep2, x2, _ = fresh.step(idx)
            finally:
                fresh.close()
            assert np.array_equal(_bits(x1), _bits(x2)) and rep1 == rep2
            for b in [dx] + out:
                b.free()
    finally:
        if twin is not None:
            twin.close()
        dev.close()


def _critic_torch(case, sets, dtype, lr=1e-3):
    """(the value gradients of the first set, its value_loss, the parameters after Adam over every set, their value losses) in `dtype`"""
    import torch
    F = torch.nn.functional
    params = torch_params(case, dtype)
    vals = [params[i] for i in VALUE]
    act = torch.tanh if case["activation"] == "tanh" else torch.relu
    opt = torch.optim.Adam(vals, lr=lr, eps=1e-5)
    first, losses = None, []
    for idx in sets:
        x, R = (torch.tensor(np.asarray(case[k])[np.asarray(idx)], dtype=dtype) for k in ("obs", "returns"))
        v = F.linear(act(F.linear(act(F.linear(x, params[4], params[5])), params[6], params[7])), params[10], params[11]).flatten()
        loss = F.mse_loss(R, v)
        opt.zero_grad()
        loss.backward()
        if first is None:
            first = [p.grad.numpy().astype(np.float64).copy() for p in vals]
        opt.step()
        losses.append(float(loss.detach()))
    return first, [p.detach().numpy().astype(np.float64) for p in params], np.array(losses)


@pytest.mark.parametrize("kind,activation", [("pst", "tanh"), ("ppl", "relu")])
def test_critic_gradient_and_three_adam_minibatches(engines, kind, activation):
    import torch
    from ev2gym_amd.trpo import value_grad_numpy
    eng, (D, P) = engines[kind], SHAPES[kind]
    n_rows = N_ROWS[activation]
    case = make_case(D, P, activation=activation, n_rows=n_rows)
    rng = np.random.default_rng(21)
    sets = [rng.choice(n_rows, B, replace=False) for B in (64, 95, 33)]
    g64, ref, l64 = _critic_torch(case, sets, torch.float64)
    g32, y32, l32 = _critic_torch(case, sets, torch.float32)
    vl_np, g_np = value_grad_numpy(case["weights"], case["obs"], case["returns"], sets[0], activation=activation)
    assert abs(vl_np - l64[0]) <= 1e-12 * max(1.0, l64[0]) and all(np.abs(a - b).max() <= 1e-10 * np.abs(b).max() for a, b in zip(g_np, g64))
    dev = _Trpo(eng, case)
    try:
        start = dev.weights()
        losses = [dev.critic(sets[0])]
        got_g = dev.eng.ppo_get_grads(dev.trpo, _shape(case))
        tag = f"CRITIC {kind} {activation}"
        ok = True
        for k, i in enumerate(VALUE):
            ok &= _vec(tag, "d value_loss / d " + NAMES[i], got_g[i].astype(np.float64), g64[k], g32[k])
        losses += [dev.critic(ix) for ix in sets[1:]]
        ok &= _val(tag, "value_loss of the three minibatches", losses, l64, l32)
        got = dev.weights()
        for i in VALUE:
            ok &= _val(tag, NAMES[i], got[i], ref[i], y32[i])
            assert not np.array_equal(got[i], start[i]), NAMES[i]
        for i in ACTOR:   # the actor's arrays, and their images: the mean of a fresh policy made from the start's arrays
            assert np.array_equal(_bits(got[i]), _bits(start[i])), NAMES[i]
        assert ok
    finally:
        dev.close()


def test_the_same_calls_give_the_same_bits_and_the_images_follow(engines):
    from ev2gym_amd.engine import trpo_query
    from ev2gym_amd.onpolicy import GaussianActorCritic
    eng, (D, P) = engines["ppl"], SHAPES["ppl"]
    case = make_case(D, P, n_rows=600)
    sets = _index_sets(trpo_query(*_shape(case))["grid_cap"], 600)
    runs, fresh = [], None
    try:
        for _ in range(2):   # two fresh learners, the same calls
            dev = _Trpo(eng, case)
            try:
                rep, x, g = dev.step(sets[5])
                vl = [dev.critic(ix) for ix in (sets[5], sets[3], sets[1])]
                runs.append((rep, x, g, vl, dev.weights()))
                if len(runs) == 2:
                    assert rep["accepted"]
                    # the repacked images: a second policy object created from the read-back arrays computes the same bits
                    eng.ppo_sync(dev.trpo)
                    w = runs[1][4]
                    fresh = GaussianActorCritic(w[:12], w[12], activation="tanh", lo=-1.0, seed=5).attach(eng)
                    dx = _up(eng, np.concatenate([np.zeros((1, D), np.float32), case["obs"][:36]]))
                    out = [[eng.empty((37, P), np.float32), eng.empty((37,), np.float32)] for _ in range(2)]
                    acts = [[eng.empty((37, P), np.float32), eng.empty((37,), np.float32)] for _ in range(2)]
                    for ac, (m, v), (a, lp) in zip((dev.pol.ac, fresh.ac), out, acts):
                        eng.ac_forward(ac, dx, 37, mean=m, value=v)
                        eng.ac_seed(ac, 11, 3)
                        eng.ac_act(ac, dx, 37, actions=a, log_prob=lp)
                    eng.synchronize()
                    for a, b in zip(out[0] + acts[0], out[1] + acts[1]):
                        assert np.array_equal(_bits(a.to_host()), _bits(b.to_host()))
                    for b in [dx] + sum(out, []) + sum(acts, []):
                        b.free()
            finally:
                dev.close()
        (ra, xa, ga, va, wa), (rb, xb, gb, vb, wb) = runs
        assert ra == rb and np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ga), _bits(gb))
        assert np.array_equal(_bits(np.array(va)), _bits(np.array(vb)))
        for name, a, b, w0 in zip(NAMES, wa, wb, list(case["weights"]) + [case["log_std"]]):
            assert np.array_equal(_bits(a), _bits(b)), name
            assert not np.array_equal(a, w0), name   # (the step and the critic moved every array)
    finally:
        if fresh is not None:
            fresh.close()


# ---- TRPOLearner behind a collector ----
def _torch_rounds(cases, pieces, dtype, w0, ls0, lr=1e-3):
    """The loop a torch user has today over the collected rounds: TorchTrpo's policy step on every row, then Adam(eps=1e-5) on the value arrays
    over the round's minibatches.  (final parameters, per round: the step's dict and the mean value loss)"""
    import torch
    F = torch.nn.functional
    params = torch_params(dict(weights=w0, log_std=ls0), dtype)
    vals = [params[i] for i in VALUE]
    opt = torch.optim.Adam(vals, lr=lr, eps=1e-5)
    steps, vls = [], []
    for case, sets in zip(cases, pieces):
        N = case["obs"].shape[0]
        steps.append(TorchTrpo(case, np.arange(N), dtype, params=params).step())
        losses = []
        for idx in sets:
            x, R = (torch.tensor(case[k][idx], dtype=dtype) for k in ("obs", "returns"))
            v = F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, params[4], params[5])), params[6], params[7])), params[10], params[11]).flatten()
            loss = F.mse_loss(R, v)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        vls.append(float(np.mean(losses)))
    return [p.detach().numpy().astype(np.float64) for p in params], steps, vls


def test_train_and_learn_end_to_end_behind_a_collector():
    import torch
    from ev2gym_amd.onpolicy import SB3_KEYS, SB3_LOG_STD, GaussianActorCritic, OnPolicyCollector, init_ac_weights
    from ev2gym_amd.trpo import TRPOLearner
    eng = _gen_engine("pst", pool=3)
    w0, ls0 = init_ac_weights(eng.D, eng.P, seed=3), np.full(eng.P, -0.5, np.float32)
    pol = GaussianActorCritic(w0, ls0, lo=0.0, seed=5).attach(eng)
    try:
        col = OnPolicyCollector(eng, pol, n_steps=5)
        learner = TRPOLearner(col, batch_size=64, n_critic_updates=2)
        N = 5 * eng.E
        rng = np.random.default_rng(8)
        cases, pieces, stats = [], [], []
        for _ in range(3):
            batch = col.collect().clone()
            perms = [rng.permutation(N) for _ in range(2)]
            sets = [p[i:i + 64] for p in perms for i in range(0, N, 64)]
            stats.append(learner.train(batch, minibatches=sets))
            f = lambda t, *s: t.reshape(-1, *s).cpu().numpy()  # noqa: E731
            cases.append(dict(activation="tanh", obs=f(batch.observations, pol.d_in), actions=f(batch.actions, pol.d_out), old_log_prob=f(batch.log_probs),
                              advantages=f(batch.advantages), returns=f(batch.returns)))
            pieces.append(sets)
        ref, ref_steps, ref_vl = _torch_rounds(cases, pieces, torch.float64, w0, ls0)
        y32, y32_steps, y32_vl = _torch_rounds(cases, pieces, torch.float32, w0, ls0)
        for k, (r, y) in enumerate(zip(ref_steps, y32_steps)):
            oks, mk, mj = decisions(r, 0.01)
            _record(f"TRPO END-TO-END round {k}: tries {r['tries']}  margins {mk:.3e} {mj:.3e}  iterations {r['cg_iterations']}")
            assert mk >= 1e-3 and mj >= 1e-4 and decisions(y, 0.01)[0] == oks and r["cg_iterations"] == y["cg_iterations"] == 15
        sd = learner.state_dict()
        got = [sd[k] for k in SB3_KEYS] + [sd[SB3_LOG_STD]]
        ok = True
        for name, g, r, y in zip(NAMES, got, ref, y32):
            ok &= _val("END-TO-END", name, g, r, y)
        for k, (s, r, y) in enumerate(zip(stats, ref_steps, y32_steps)):
            assert s["is_line_search_success"] == r["accepted"] and s["line_search_tries"] == r["line_search_tries"] and s["cg_iterations"] == 15
            ok &= _val(f"END-TO-END round {k}", "policy_objective", s["policy_objective"], r["objective_before"], y["objective_before"])
            ok &= _val(f"END-TO-END round {k}", "kl_divergence_loss", s["kl_divergence_loss"], r["kl"] if r["accepted"] else 0.0, y["kl"] if y["accepted"] else 0.0)
            ok &= _val(f"END-TO-END round {k}", "value_loss", s["value_loss"], ref_vl[k], y32_vl[k])
        assert ok
        # repeated critic passes on the last batch: the value loss falls
        first = learner.train(batch, minibatches=[np.arange(N)] * 1)["value_loss"]
        for _ in range(3):
            last = learner.train(batch, minibatches=[np.arange(N)] * 20)["value_loss"]
        _record(f"TRPO SANITY value_loss over repeated critic passes on one batch: {first:.6e} -> {last:.6e}")
        assert np.isfinite(last) and last < first
        # learn(): one more round with the learner's own permutations
        out = learner.learn(N)
        assert len(out) == 1 and set(out[0]) == {"policy_objective", "kl_divergence_loss", "value_loss", "is_line_search_success", "line_search_tries", "cg_iterations"}
        assert np.isfinite(out[0]["value_loss"]) and learner.num_timesteps == N
        learner.close()
    finally:
        pol.close()
        eng.close()


# ---- refusals ----
def test_refusals_through_the_abi(engines):
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.onpolicy import GaussianActorCritic, init_ac_weights
    eng = engines["pst"]
    case = make_case(eng.D, eng.P, n_rows=64)
    dev = _Trpo(eng, case)

    def refused(code, word, fn, *a, **kw):
        with pytest.raises(EngineError) as e:
            fn(*a, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)

    other = None
    try:
        ix = _up(eng, np.arange(8, dtype=np.int32))
        rows = (dev.obs, dev.actions, dev.old, dev.adv)
        # a report or a direction before any policy step
        refused(STATE, "no policy step", eng.trpo_get_report, dev.trpo)
        refused(STATE, "no policy step", eng.trpo_get_direction, dev.trpo, dev.n_actor)
        for k in range(4):
            bad = list(rows)
            bad[k] = None
            refused(ARG, "null", eng.trpo_grad, dev.trpo, *bad, ix, 8)
            refused(ARG, "null", eng.trpo_policy_step, dev.trpo, *bad, ix, 8)
        refused(ARG, "null", eng.trpo_policy_step, dev.trpo, *rows, None, 8)
        refused(ARG, "null", eng.trpo_fvp, dev.trpo, dev.obs, ix, 8, None, dev.hv)
        refused(ARG, "null", eng.trpo_critic_minibatch, dev.trpo, dev.obs, None, ix, 8)
        refused(ARG, "null", eng.trpo_policy_step, None, *rows, ix, 8)
        refused(ARG, "B must be", eng.trpo_policy_step, dev.trpo, *rows, ix, 0)
        refused(ARG, "B must be", eng.trpo_critic_minibatch, dev.trpo, dev.obs, dev.ret, ix, -3)
        refused(ARG, "lr", eng.trpo_set_rate, dev.trpo, float("nan"))
        refused(ARG, "lr", eng.trpo_set_rate, dev.trpo, -1.0)
        # a second learner of any kind
        for create in (eng.trpo_create, eng.ppo_create, eng.a2c_create):
            refused(STATE, "already has a learner", create, dev.pol.ac)
        # the other kinds' entries on a TRPO learner
        refused(STATE, "TRPO learner", eng.ppo_grad, dev.trpo, *rows, dev.ret, ix, 8)
        refused(STATE, "TRPO learner", eng.ppo_apply, dev.trpo)
        refused(STATE, "TRPO learner", eng.ppo_set_rates, dev.trpo, 3e-4, 0.2)
        refused(STATE, "TRPO learner", eng.a2c_update, dev.trpo, dev.obs, dev.actions, dev.adv, dev.ret, ix, 8)
        refused(STATE, "TRPO learner", eng.a2c_set_rate, dev.trpo, 7e-4)
        # ... and TRPO's entries on a PPO and on an A2C learner
        other = GaussianActorCritic(case["weights"], case["log_std"]).attach(eng)
        for create, word in ((eng.ppo_create, "PPO learner"), (eng.a2c_create, "A2C learner")):
            lrn = create(other.ac)
            refused(STATE, word, eng.trpo_policy_step, lrn, *rows, ix, 8)
            refused(STATE, word, eng.trpo_grad, lrn, *rows, ix, 8)
            refused(STATE, word, eng.trpo_fvp, lrn, dev.obs, ix, 8, dev.v, dev.hv)
            refused(STATE, word, eng.trpo_critic_minibatch, lrn, dev.obs, dev.ret, ix, 8)
            refused(STATE, word, eng.trpo_set_rate, lrn, 1e-3)
            refused(STATE, word, eng.trpo_get_report, lrn)
            eng.ppo_destroy(lrn)
        # out-of-range config values, the field named; a network the plan refuses
        for kw, word in ((dict(lr=-1e-3), "lr"), (dict(lr=float("inf")), "lr"), (dict(target_kl=0.0), "target_kl"), (dict(target_kl=float("nan")), "target_kl"),
                         (dict(cg_damping=-0.1), "cg_damping"), (dict(cg_max_steps=0), "cg_max_steps"), (dict(line_search_max_iter=0), "line_search_max_iter"),
                         (dict(line_search_shrinking_factor=0.0), "line_search_shrinking_factor"),
                         (dict(line_search_shrinking_factor=1.0), "line_search_shrinking_factor"),
                         (dict(line_search_shrinking_factor=float("nan")), "line_search_shrinking_factor")):
            refused(ARG, word, eng.trpo_create, other.ac, **kw)
        wide = GaussianActorCritic(init_ac_weights(eng.D, eng.P, h=(256, 256), v=(256, 256)), case["log_std"]).attach(eng)
        refused(ARG, "256 is too wide", eng.trpo_create, wide.ac)
        wide.close()
        # destroying the policy destroys the learner
        lrn = eng.trpo_create(other.ac)
        other.close()
        other = None
        refused(ARG, "not created on this handle", eng.trpo_get_report, lrn)
        # the learner is as it was: a step, a report
        eng.trpo_policy_step(dev.trpo, *rows, ix, 8)
        assert eng.trpo_get_report(dev.trpo)["cg_iterations"] >= 1
        ix.free()
    finally:
        if other is not None:
            other.close()
        dev.close()
