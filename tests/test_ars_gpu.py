"""The ARS learner on the device (csrc/ev2g_ars.h; ev2g_ars_*; ev2gym_amd/ars.py): the population actor against a float64 numpy forward on every
row's OWN candidate, candidate indexing bit for bit, perturb and update against their host twins bit for bit, a whole episode in population mode
against a twin engine and the returns' host twin, three train() iterations against the twin loop, the refusals and the teardown.
These are the workload's own shapes; tests/test_ars_range_gpu.py runs the same kernels over the rest of the range the plan accepts.

Engines: the PublicPST fixture tests/golden/pst_rand_s2 tiled to pools of 12 envs (and 8) x 20 ports, 112-step episodes (ev2g_step_wave; both
collector routes) -- a short generated pool sees its first EV only around step 11, so its rewards are all zero and its returns check nothing.  Forward tolerance, per
case: d32 = the largest deviation of a torch-CPU float32 forward from the float64 forward on the same rows and weights; the device gets
4 d32 + 4 * 2^-23 * max(1, |y|) (tests/test_onpolicy_gpu.py's idiom).  Every figure is printed before it is asserted.

The forward cases draw theta at torch.nn.Linear's initial scale and perturb it with delta_std 0.1, so that the layers' pre-activations are of
order 1: with weights several times larger the 256-wide networks saturate tanh on most ports (an action of exactly 0 or 1 checks nothing) and d32,
taken from as few as R = 1 rows, becomes a yardstick of a handful of unsaturated elements with pre-activations in the tens."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden
from tests import ars_cases as ac

pytestmark = pytest.mark.gpu

ARG, STATE, DONE = -1, -3, -4
EPS32 = 2.0 ** -23
E_GEN = 12


def _engine(pool=1, n_envs=E_GEN):
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    _, batch, rk, sk = load_golden(os.path.join(GOLDEN_DIR, "pst_rand_s2.npz"))
    eng = Engine(batch.tile(n_envs * pool), rk, sk, device=0, flags=_abi.FLAG_LOG_SOC, n_active_envs=n_envs)
    assert (eng.E, eng.M, eng.D, eng.P) == (n_envs, n_envs * pool, 63, 20) and eng.kernel_name.startswith("ev2g_step_wave")
    return eng


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _record(line):
    """A figure of this run: printed, and appended to the file EV2G_ARS_RECORD names when it is set."""
    print(line)
    path = os.environ.get("EV2G_ARS_RECORD")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _create(eng, tag, lo, n_delta, theta="random", seed=5, **cfg):
    kind, D, h1, h2, P = ac.NETS[tag]
    th = ac.random_theta(tag) if isinstance(theta, str) else theta
    cfg.setdefault("n_top", n_delta)
    return eng.ars_create(kind, D, h1, h2, P, lo, th, seed=seed, n_delta=n_delta, **cfg), th


def _act(eng, a, x, P, population):
    n = x.shape[0]
    dx, da = eng.empty(x.shape, np.float32).upload(x), eng.empty((n, P), np.float32)
    try:
        eng.ars_act(a, dx, n, da, population=population)
        eng.synchronize()
        return da.to_host()
    finally:
        dx.free()
        da.free()


def _torch32(x, arrays, kind, lo):
    import torch
    F = torch.nn.functional
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
    X = torch.from_numpy(x)
    with torch.no_grad():
        if kind == "LinearPolicy":
            return torch.clamp(F.linear(X, t[0]), lo, 1.0).numpy()
        a = torch.tanh(F.linear(torch.relu(F.linear(torch.relu(F.linear(X, t[0], t[1])), t[2], t[3])), t[4], t[5]))
        return (0.5 * (a + 1.0) if lo == 0.0 else a).numpy()


# ---- the population forward ----
@pytest.mark.parametrize("lo", [-1.0, 0.0])
@pytest.mark.parametrize("tag", sorted(ac.NETS))
def test_population_forward_on_every_rows_own_candidate(eng, tag, lo):
    from ev2gym_amd.ars import ars_forward_numpy, split_theta
    kind, D, h1, h2, P = ac.NETS[tag]
    rng = np.random.default_rng(D + P + int(lo))
    rows = rng.normal(size=(65, D)).astype(np.float32)
    for C in (2, 4, 6):
        a, _ = _create(eng, tag, lo, C // 2, delta_std=0.1)
        try:
            eng.ars_perturb(a)
            n_params = sum(int(np.prod(s)) for s in __import__("ev2gym_amd")._abi.ars_param_shapes(kind, D, h1, h2, P))
            cands = [split_theta(eng.ars_get_candidate(a, c, n_params), kind, D, h1, h2, P) for c in range(C)]
            for R in (1, 31, 32, 33, 65):
                x = np.tile(rows[:R], (C, 1))   # every candidate sees the same rows: what differs is the weights
                ref = np.stack([ars_forward_numpy(rows[:R], cands[c], kind, lo) for c in range(C)])
                d32 = max(float(np.abs(_torch32(rows[:R], cands[c], kind, lo) - ref[c]).max()) for c in range(C))
                tol = 4.0 * d32 + 4.0 * EPS32 * np.maximum(1.0, np.abs(ref))
                apart = min(float(np.abs(ref[c] - ref[c2]).max()) for c in range(C) for c2 in range(c))
                got = _act(eng, a, x, P, True).reshape(C, R, P)
                err = np.abs(got - ref)
                _record(f"ARS FORWARD {tag} lo {lo:g} C {C} R {R}: d32 {d32:.3e}  |act - f64| {err.max():.3e} (tol {tol.min():.3e})  candidates apart {apart:.3e}")
                assert apart > float(tol.max()), "the candidates' float64 actions must differ by more than the tolerance"
                assert np.isfinite(got).all() and (err <= tol).all()
                assert got.min() >= lo and got.max() <= 1.0
        finally:
            eng.ars_destroy(a)


# ---- candidate indexing ----
@pytest.mark.parametrize("tag", ["pst-33-17", "ppl-linear"])
def test_a_candidates_rows_equal_a_centre_launch_of_its_weights_bit_for_bit(eng, tag):
    kind, D, h1, h2, P = ac.NETS[tag]
    C, R = 6, 33
    rng = np.random.default_rng(12)
    x = rng.normal(size=(C * R, D)).astype(np.float32)
    a, theta = _create(eng, tag, -1.0, C // 2, delta_std=0.1)
    others = []
    try:
        eng.ars_perturb(a)
        pop = _act(eng, a, x, P, True).reshape(C, R, P)
        small = np.concatenate([x[c * R + 20:c * R + 25] for c in range(C)])   # five rows of every candidate, at another place of another tile
        pop5 = _act(eng, a, small, P, True).reshape(C, 5, P)
        for c in range(C):
            b, _ = _create(eng, tag, -1.0, 1, theta=eng.ars_get_candidate(a, c, theta.size))
            others.append(b)
            assert np.array_equal(_bits(_act(eng, b, x[c * R:(c + 1) * R], P, False)), _bits(pop[c])), c
            assert np.array_equal(_bits(pop5[c]), _bits(pop[c, 20:25])), c
        assert not np.array_equal(_bits(pop[0]), _bits(_act(eng, others[1], x[:R], P, False)))   # (another candidate's weights give other bits)
    finally:
        for b in others + [a]:
            eng.ars_destroy(b)


# ---- perturb ----
@pytest.mark.parametrize("tag", ["pst-33-17", "pst-linear"])
def test_perturb_equals_the_host_twin_and_leaves_the_centre_alone(eng, tag):
    from ev2gym_amd.engine import host_ars_perturb
    kind, D, h1, h2, P = ac.NETS[tag]
    n_delta, seed, std = 3, 19, 0.05
    a, theta = _create(eng, tag, 0.0, n_delta, seed=seed, delta_std=std)
    x = np.random.default_rng(6).normal(size=(40, D)).astype(np.float32)
    try:
        centre = _act(eng, a, x, P, False)
        for it, (s, first) in enumerate(((seed, None), (seed, None), (23, 7))):
            if first is not None:
                eng.ars_seed(a, s, first)
            n_it = it if first is None else first
            eng.ars_perturb(a)
            delta, cand = host_ars_perturb(theta, n_delta, std, s, n_it)
            assert np.array_equal(_bits(eng.ars_get_deltas(a, n_delta, theta.size)), _bits(delta)), it
            for c in range(2 * n_delta):
                assert np.array_equal(_bits(eng.ars_get_candidate(a, c, theta.size)), _bits(cand[c])), (it, c)
            assert np.array_equal(_bits(_act(eng, a, x, P, False)), _bits(centre)), it
            assert eng.ars_counters(a)[0] == n_it + 1
        assert np.array_equal(_bits(eng.ars_get_weights(a, theta.size)), _bits(theta))
    finally:
        eng.ars_destroy(a)


# ---- update ----
@pytest.mark.parametrize("name", ["plain", "ties", "equal", "nan", "inf"])
def test_update_on_set_returns_equals_the_host_twin(eng, name):
    from ev2gym_amd.engine import host_ars_update
    tag, n_delta, n_top, lr = "pst-33-17", 4, (2 if name == "ties" else 4), 0.02
    kind, D, h1, h2, P = ac.NETS[tag]
    returns = ac.crafted_returns(n_delta)[name]
    a, theta = _create(eng, tag, -1.0, n_delta, n_top=n_top, learning_rate=lr)
    x = np.random.default_rng(8).normal(size=(33, D)).astype(np.float32)
    b = None
    try:
        before = _act(eng, a, x, P, False)
        eng.ars_perturb(a)
        delta = eng.ars_get_deltas(a, n_delta, theta.size)
        eng.ars_set_returns(a, returns)
        eng.ars_update(a)
        rep = eng.ars_get_report(a, n_delta)
        want, wrep = host_ars_update(theta, delta, returns, n_top, lr)
        new = eng.ars_get_weights(a, theta.size)
        _record(f"ARS UPDATE {name}: sigma_R {rep['sigma_r']:.6g} step {rep['step']:.6g} refused {rep['refused']} first_bad {rep['first_bad']}")
        assert np.array_equal(_bits(new), _bits(want))
        assert np.array_equal(rep["ranks"], wrep["ranks"]) and np.array_equal(_bits(rep["returns"]), _bits(returns))
        assert _bits(np.float64(rep["sigma_r"])) == _bits(np.float64(wrep["sigma_r"])) and _bits(np.float64(rep["step"])) == _bits(np.float64(wrep["step"]))
        assert (rep["refused"], rep["first_bad"], rep["n_top"], rep["iteration"]) == (wrep["refused"], wrep["first_bad"], n_top, 0)
        after = _act(eng, a, x, P, False)
        if name in ("nan", "inf", "equal"):
            assert rep["refused"] == (name != "equal") and np.array_equal(_bits(new), _bits(theta)) and np.array_equal(_bits(after), _bits(before))
        else:
            assert not rep["refused"] and (new != theta).any()
            b, _ = _create(eng, tag, -1.0, 1, theta=new)   # the centre image was repacked from the new theta
            assert np.array_equal(_bits(after), _bits(_act(eng, b, x, P, False))) and not np.array_equal(_bits(after), _bits(before))
        assert eng.ars_counters(a)[1] == 1
    finally:
        eng.ars_destroy(a)
        if b:
            eng.ars_destroy(b)


# ---- rollout ----
def _obs_of(eng, a):
    out = np.empty((eng.E, eng.D), np.float32)
    eng.synchronize()
    eng.memcpy_d2h(out, eng.ars_obs_f32(a), out.nbytes)
    return out


@pytest.mark.parametrize("tag", ["pst-33-17", "pst-linear"])
def test_a_population_episode_against_a_twin_engine_and_the_returns_twin(eng, tag):
    from ev2gym_amd.engine import host_ars_returns
    kind, D, h1, h2, P = ac.NETS[tag]
    E, T, n_delta, seed, offset = eng.E, eng.T, 2, 4, -0.5   # C = 4, R = 3
    a, theta = _create(eng, tag, 0.0, n_delta, seed=seed, delta_std=0.3, alive_bonus_offset=offset)
    twin = _engine()
    rew = eng.empty((T, E))
    try:
        assert eng.ars_obs_f32(a) and eng.ars_actions_f32(a)
        eng.ars_perturb(a)
        eng.reset_f32(eng.ars_obs_f32(a), 0)
        x_obs, x_act = twin.empty((E, D), np.float32), twin.empty((E, P), np.float32)
        t_rew, t_done, t_mask = twin.empty((E,)), twin.empty((E,), np.uint8), twin.empty((E, P), np.uint8)
        twin.set_extras(obs_f32=x_obs, actions_f32=x_act)
        twin.reset_f32(x_obs, 0)
        twin.synchronize()
        rows = []
        for t in range(T):   # the episode step by step: every step's observation, action and reward against the twin
            obs = _obs_of(eng, a)
            assert np.array_equal(_bits(obs), _bits(x_obs.to_host())), t
            x_act.upload(_act(eng, a, obs, P, True))
            eng.ars_rollout(a, 1, population=True, reward=rew.at(t * E), r_stride=E)
            twin.step_n(1, None, 0, None, 0, t_rew, 0, t_done, 0, t_mask, 0, auto_reset=False, persistent=False)
            twin.synchronize()
            rows.append(t_rew.to_host())
        eng.synchronize()
        kept = rew.to_host()
        assert np.array_equal(_bits(kept), _bits(np.stack(rows))) and np.abs(kept).max() > 0 and t_done.to_host().all() and eng.current_step == T
        assert np.array_equal(_bits(_obs_of(eng, a)), _bits(x_obs.to_host()))
        env = np.zeros(E)
        host_ars_returns(env, kept)
        want = host_ars_returns(env, None, 2 * n_delta, offset, T)
        stepwise = eng.ars_get_env_returns(a)
        assert np.array_equal(_bits(stepwise), _bits(env)) and eng.ars_counters(a)[2] == T
        eng.ars_update(a)
        rep = eng.ars_get_report(a, n_delta)
        _record(f"ARS ROLLOUT {tag}: candidate returns {rep['returns']}")
        assert np.array_equal(_bits(rep["returns"]), _bits(want)) and len(set(rep["returns"].tolist())) > 1
        # the same candidates again: one call, two segments, and the registered hand-over route give the same returns
        h_obs, h_act = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
        for how in ("one call", "two segments", "registered route"):
            eng.ars_set_weights(a, theta)
            eng.ars_seed(a, seed, 0)
            eng.ars_perturb(a)
            if how == "registered route":
                eng.set_extras(obs_f32=h_obs, actions_f32=h_act)
            eng.reset_f32(eng.ars_obs_f32(a), 0)
            for k in ((5, T - 5) if how == "two segments" else (T,)):
                eng.ars_rollout(a, k, population=True)
            assert np.array_equal(_bits(eng.ars_get_env_returns(a)), _bits(env)), how
            assert np.array_equal(_bits(_obs_of(eng, a)), _bits(x_obs.to_host())), how
            eng.set_extras()
    finally:
        eng.set_extras()
        eng.ars_destroy(a)
        rew.free()
        twin.close()


# ---- end to end ----
@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("policy", ["MlpPolicy", "LinearPolicy"])
def test_three_iterations_equal_the_twin_loop(policy, rounds):
    from ev2gym_amd.ars import ARSLearner, ars_iteration_host
    n_delta, lr, std, seed, offset = 2, 0.02, 0.05, 11, 0.25
    eng, twin = _engine(pool=3), _engine(pool=3)
    E, M = eng.E, eng.M
    kw = dict(policy=policy, n_delta=n_delta, learning_rate=lr, delta_std=std, alive_bonus_offset=offset, n_eval_episodes=rounds * E // (2 * n_delta), seed=seed,
              net_arch=(33, 17), lo=0.0)
    try:
        learner = ARSLearner(eng, **kw)
        assert learner.rounds == rounds
        zero = learner.predict(np.random.default_rng(1).normal(size=(7, eng.D)))
        assert np.array_equal(zero, np.full((7, eng.P), 0.5 if policy == "MlpPolicy" else 0.0, np.float32))   # unscale(tanh(0)) / clip(0)
        pol = learner.policy
        twin_ars = twin.ars_create(pol.KIND, pol.d_in, pol.h1, pol.h2, pol.d_out, 0.0, None, seed=seed, n_delta=n_delta, n_top=n_delta)
        theta, off, thetas = np.zeros(pol.n_params, np.float32), eng.scenario_offset, []
        for it in range(3):
            rep = learner.train()
            offsets = [(off + (r + 1) * E) % M for r in range(rounds)]
            off = offsets[-1]
            theta, want, _ = ars_iteration_host(twin, twin_ars, theta, it, offsets, n_delta, n_delta, lr, std, offset, seed)
            got = eng.ars_get_weights(learner.ars, pol.n_params)
            _record(f"ARS TRAIN {policy} rounds {rounds} iteration {it}: returns {rep['returns']} sigma_R {rep['sigma_r']:.6g} step {rep['step']:.6g}")
            assert np.array_equal(_bits(rep["returns"]), _bits(want["returns"])) and np.array_equal(rep["ranks"], want["ranks"])
            assert (rep["sigma_r"], rep["step"], rep["refused"], rep["iteration"]) == (want["sigma_r"], want["step"], False, it)
            assert np.array_equal(_bits(got), _bits(theta)) and np.isfinite(got).all()
            thetas.append(got)
        assert (thetas[0] != 0).any() and (thetas[2] != thetas[0]).any() and learner.num_timesteps == 3 * rounds * eng.T * E
        learner.close()
        # a fresh learner with the same seed on the same windows repeats the run bit for bit; learn() runs
        eng.reset(offset=0)
        again = ARSLearner(eng, **kw)
        reports = again.learn(3 * rounds * eng.T * E)
        assert len(reports) == 3 and np.array_equal(_bits(again.get_weights()), _bits(thetas[2]))
        assert np.array_equal(_bits(again.policy.theta()), _bits(thetas[2])) and np.isfinite(again.evaluate(1))
        again.close()
    finally:
        eng.close()
        twin.close()


# ---- refusals ----
def test_refusals_leave_the_handle_usable(eng):
    from ev2gym_amd.engine import EngineError
    a, theta = _create(eng, "pst-33-17", 0.0, 2)
    odd, _ = _create(eng, "pst-33-17", 0.0, 5)           # 12 envs are no multiple of 10
    wide, _ = _create(eng, "ppl-linear", 0.0, 2)         # 162 -> 50 on a 63 -> 20 engine
    dx, da = eng.empty((12, 63), np.float32), eng.empty((12, 20), np.float32)

    def refused(code, word, call, *args, **kw):
        with pytest.raises(EngineError, match=word) as e:
            call(*args, **kw)
        assert e.value.code == code, (e.value.code, code)

    try:
        eng.reset_f32(eng.ars_obs_f32(a), 0)
        refused(STATE, "ev2g_ars_perturb first", eng.ars_rollout, a, 1)
        refused(STATE, "ev2g_ars_perturb first", eng.ars_act, a, dx, 12, da, population=True)
        refused(STATE, "no directions yet", eng.ars_update, a)
        for obj in (a, odd, wide):
            eng.ars_perturb(obj)
        refused(STATE, "no returns yet", eng.ars_update, a)
        refused(ARG, "not a positive multiple of 2 n_delta", eng.ars_rollout, odd, 1)
        refused(ARG, "not a positive multiple of 2 n_delta", eng.ars_act, odd, dx, 12, da, population=True)
        refused(ARG, "d_in 162 != the observation width 63", eng.ars_rollout, wide, 1)
        refused(DONE, "past the episode end", eng.ars_rollout, a, eng.T + 1)
        refused(ARG, "reward stride", eng.ars_rollout, a, 1, reward=da, r_stride=eng.E - 1)
        refused(ARG, "candidate 4 is outside", eng.ars_get_candidate, a, 4, theta.size)
        refused(ARG, "delta_std must be finite and > 0", eng.ars_set_rates, a, 0.02, 0.0)
        bad = theta.copy()
        bad[3] = np.nan
        refused(ARG, "theta\\[3\\] is not finite", eng.ars_set_weights, a, bad)
        assert eng.current_step == 0
        eng.ars_rollout(odd, 2, population=False)          # the centre policy needs no multiple
        eng.ars_rollout(a, eng.T - 2)
        eng.ars_update(a)
        rep = eng.ars_get_report(a, 2)
        assert not rep["refused"] and eng.current_step == eng.T and (eng.ars_get_weights(a, theta.size) != theta).any()
        refused(STATE, "no returns yet", eng.ars_update, a)
    finally:
        for obj in (a, odd, wide):
            eng.ars_destroy(obj)
        dx.free()
        da.free()


# ---- teardown ----
def test_destroy_and_close_with_a_live_object():
    from ev2gym_amd.engine import EngineError
    eng, far = _engine(), _engine(n_envs=8)
    a, theta = _create(eng, "pst-64-64", -1.0, 2)
    b, _ = _create(eng, "pst-linear", -1.0, 2)
    eng.ars_perturb(a)
    eng.reset_f32(eng.ars_obs_f32(a), 0)
    eng.ars_rollout(a, 2)
    far.ars_destroy(a)   # another handle's destroy is nothing
    with pytest.raises(EngineError, match="not created on this handle") as e:
        far.ars_perturb(a)
    assert e.value.code == ARG
    eng.ars_rollout(a, 1)
    eng.ars_destroy(b)
    with pytest.raises(EngineError, match="not created on this handle"):
        eng.ars_perturb(b)
    eng.ars_destroy(b)   # a second destroy is nothing
    eng.ars_update(a)
    assert not eng.ars_get_report(a, 2)["refused"]
    eng.synchronize()
    eng.check_faults()
    eng.close()          # with `a` alive: the handle frees it
    far.close()
