"""The ARS kernels over the whole range plan_ars accepts (csrc/ev2g_ars.h, ev2g_ars_host.h; tests/test_ars_gpu.py stops at the workload's own
shapes).  The case tables and what they rely on are tests/ars_cases.py's; tests/test_ars_cpu.py pins them on the float64 reference alone.

  * the population forward on ars_cases.EDGE_NETS -- every plan maximum, no padding at all, one past every tile, P = 57 (write-out lane 0
    takes an eighth port), 1 -> 1, both policy kinds -- with lo -1 and 0, C 2 and 6, R 1, 32 and 33, every row against the float64 forward of
    its OWN candidate (read back with ars_get_candidate) under tests/test_ars_gpu.py's tolerance, 4 d32 + 4 * 2^-23 * max(1, |y|) with d32
    from torch-CPU float32 on the same rows and weights; the linear policies' clipped elements exactly lo or 1; a saturated MLP whose every
    second port is exactly 1 or lo;
  * many candidates: 8192 candidates of one row (8192 workgroups, `images + cand * stride` up to cand 8191) and 514 candidates of 33 rows (two
    tiles per candidate), the candidates bit for bit the host twin's, every row under the idiom, the last candidate's rows bit for bit a centre
    launch of its weights;
  * the update at n_delta 255 .. 4096 from set returns (the rank kernel's k += 256 loop, order[] from up to 4096 threads, ars_first_bad past
    index 7): theta, ranks, sigma_R, step, refused, first_bad and n_top bit for bit host_ars_update's, the ranks numpy's stable argsort, theta
    within one float32 rounding of the float64 update, bad returns leaving theta's and the centre launch's bits alone;
  * whole population episodes with R = 33 envs per candidate (two tiles inside the step chain) and with 258 candidates (a second block of the
    candidates kernel, three of the returns kernel at E 516), against the returns' twin and, per candidate, a centre episode of its weights;
  * the contract that a centre-policy rollout changes neither the returns, the step count nor the outcome of an iteration -- as a rollout
    between perturb and update, as ARSLearner.evaluate() between two train() calls, and as a centre segment between an iteration's rounds;
  * ars_set_rates: the next perturb's candidates under the new delta_std, the next update's step under the new learning rate.

Every figure is printed (and recorded, EV2G_ARS_RECORD) before it is asserted.  No tolerance comes from the device's output."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden
from tests import ars_cases as ac
from tests.test_ars_gpu import EPS32, _act, _bits, _engine, _record, _torch32

pytestmark = pytest.mark.gpu

TINY32 = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _create(eng, tag, lo, n_delta, theta, seed=ac.EDGE_SEED, **cfg):
    kind, D, h1, h2, P = ac.net_of(tag)
    cfg.setdefault("n_top", n_delta)
    return eng.ars_create(kind, D, h1, h2, P, lo, theta, seed=seed, n_delta=n_delta, **cfg)


def _idiom(rows, cands, ref, tag, lo, shared=True):
    """tests/test_ars_gpu.py's tolerance against ref [C, R, P], the float64 actions under cands [C, n_params] of rows [R, D] that every candidate
    sees (shared) or of rows [C R, D], candidate c's own at [c R, (c + 1) R): (d32, tol [C, R, P])"""
    from ev2gym_amd.ars import split_theta
    kind, D, h1, h2, P = ac.net_of(tag)
    C, R = ref.shape[:2]
    assert rows.shape[0] == (R if shared else C * R)
    d32 = max(float(np.abs(_torch32(rows if shared else rows[c * R:(c + 1) * R], split_theta(cands[c], kind, D, h1, h2, P), kind, lo) - ref[c]).max()) for c in range(C))
    return d32, 4.0 * d32 + 4.0 * EPS32 * np.maximum(1.0, np.abs(ref))


# ---- the population forward at the edges ----
@pytest.mark.parametrize("lo", [-1.0, 0.0])
@pytest.mark.parametrize("tag", sorted(ac.EDGE_NETS))
def test_population_forward_on_the_edge_networks(eng, tag, lo):
    from ev2gym_amd.ars import split_theta
    kind, D, h1, h2, P = ac.net_of(tag)
    case = ac.edge_case(tag, lo)
    assert case["misses"] == []
    rows, theta = case["rows"], case["theta"]
    for C in ac.EDGE_C:
        a = _create(eng, tag, lo, C // 2, theta, delta_std=ac.EDGE_STD)
        try:
            eng.ars_perturb(a)
            cands = np.stack([eng.ars_get_candidate(a, c, theta.size) for c in range(C)])
            assert np.array_equal(_bits(cands), _bits(case["cands"][C])), "the device's candidates are the ones the CPU module pinned"
            for R in ac.EDGE_R:
                ref = case["refs"][C, R]
                d32, tol = _idiom(rows[:R], cands, ref, tag, lo)
                apart = min(float(np.abs(ref[c] - ref[c2]).max()) for c in range(C) for c2 in range(c))
                got = _act(eng, a, np.tile(rows[:R], (C, 1)), P, True).reshape(C, R, P)
                err = np.abs(got - ref)
                _record(f"ARS EDGE FORWARD {tag} lo {lo:g} C {C} R {R}: d32 {d32:.3e}  |act - f64| {err.max():.3e} (tol {tol.min():.3e}; worst err/tol {(err / tol).max():.3f})  "
                        f"candidates apart {apart:.3e}  seeds skipped {case['seeds_skipped']}")
                assert apart > float(tol.max()), "the candidates' float64 actions must differ by more than the tolerance"
                assert np.isfinite(got).all() and (err <= tol).all()
                assert got.min() >= lo and got.max() <= 1.0
                if kind == "LinearPolicy":   # an element the reference clips, by more than the tolerance, is exactly the bound
                    raw = np.stack([rows[:R].astype(np.float64) @ split_theta(cands[c], kind, D, h1, h2, P)[0].astype(np.float64).T for c in range(C)])
                    above, below = raw > 1.0 + tol, raw < lo - tol
                    _record(f"ARS EDGE CLIP {tag} lo {lo:g} C {C} R {R}: {int(above.sum())} elements above 1, {int(below.sum())} below lo, of {raw.size}")
                    assert (got[above] == np.float32(1.0)).all() and (got[below] == np.float32(lo)).all()
                    if raw.size >= 256:
                        assert above.any() and below.any()
        finally:
            eng.ars_destroy(a)


@pytest.mark.parametrize("lo", [-1.0, 0.0])
def test_a_saturated_policy_gives_exactly_one_or_lo_on_the_shifted_ports(eng, lo):
    tag = "eighth"
    kind, D, h1, h2, P = ac.net_of(tag)
    case = ac.edge_case(tag, lo, saturate=True)
    assert case["misses"] == [] and len(case["sat"]) == 29
    up = [p for p, s in case["sat"].items() if s > 0]
    down = [p for p, s in case["sat"].items() if s < 0]
    free = [p for p in range(P) if p not in case["sat"]]
    rows, theta = case["rows"], case["theta"]
    for C in ac.EDGE_C:
        a = _create(eng, tag, lo, C // 2, theta, delta_std=ac.EDGE_STD)
        try:
            eng.ars_perturb(a)
            cands = np.stack([eng.ars_get_candidate(a, c, theta.size) for c in range(C)])
            assert np.array_equal(_bits(cands), _bits(case["cands"][C]))
            for R in ac.EDGE_R:
                ref = case["refs"][C, R]
                d32, tol = _idiom(rows[:R], cands, ref, tag, lo)
                got = _act(eng, a, np.tile(rows[:R], (C, 1)), P, True).reshape(C, R, P)
                err = np.abs(got - ref)
                _record(f"ARS EDGE SATURATED lo {lo:g} C {C} R {R}: d32 {d32:.3e}  other ports |act - f64| {err[..., free].max():.3e} (tol {tol.min():.3e}; worst err/tol "
                        f"{(err / tol)[..., free].max():.3f})  shifted ports: at 1 {int((got[..., up] == 1.0).sum())} of {got[..., up].size}, "
                        f"at lo {int((got[..., down] == lo).sum())} of {got[..., down].size}")
                assert (got[..., up] == np.float32(1.0)).all() and (got[..., down] == np.float32(lo)).all()
                assert np.isfinite(got).all() and (err[..., free] <= tol[..., free]).all()
                assert got.min() >= lo and got.max() <= 1.0
        finally:
            eng.ars_destroy(a)


# ---- many candidates ----
@pytest.mark.parametrize("name", sorted(ac.MANY))
def test_population_forward_with_many_candidates(eng, name):
    case = ac.many_case(name)
    tag, n_delta, R, C, theta, x, ref = (case[k] for k in ("tag", "n_delta", "R", "C", "theta", "x", "ref"))
    kind, D, h1, h2, P = ac.net_of(tag)
    a = _create(eng, tag, -1.0, n_delta, theta, delta_std=ac.EDGE_STD)
    b = None
    try:
        eng.ars_perturb(a)
        if C > 1000:   # the ends, the two halves' seam and 59 seeded others
            which = sorted({0, 1, n_delta - 1, n_delta, C - 1} | set(np.random.default_rng(3).choice(C, 59, replace=False).tolist()))
        else:
            which = list(range(C))
        for c in which:
            assert np.array_equal(_bits(eng.ars_get_candidate(a, c, theta.size)), _bits(case["cand"][c])), c
        d32, tol = _idiom(x, case["cand"], ref, tag, -1.0, shared=False)
        got = _act(eng, a, x, P, True).reshape(C, R, P)
        err = np.abs(got - ref)
        _record(f"ARS MANY {name} ({tag}, {C} candidates x {R} rows): d32 {d32:.3e}  |act - f64| {err.max():.3e} (tol {tol.min():.3e}; worst err/tol {(err / tol).max():.3f})  "
                f"{len(which)} candidates read back")
        assert np.isfinite(got).all() and (err <= tol).all() and got.min() >= -1.0 and got.max() <= 1.0
        b = _create(eng, tag, -1.0, 1, eng.ars_get_candidate(a, C - 1, theta.size))   # the last candidate's weights as a centre policy
        assert np.array_equal(_bits(_act(eng, b, x[(C - 1) * R:], P, False)), _bits(got[C - 1]))
        assert not np.array_equal(_bits(_act(eng, b, x[(C - 2) * R:(C - 1) * R], P, False)), _bits(got[C - 2]))   # (the neighbour ran under other weights)
    finally:
        eng.ars_destroy(a)
        if b:
            eng.ars_destroy(b)


# ---- the update at large n_delta ----
@pytest.mark.parametrize("n_delta,n_top", ac.LARGE_UPDATES)
def test_large_updates_on_set_returns_equal_the_host_twin(eng, n_delta, n_top):
    from ev2gym_amd.ars import ars_update_numpy
    from ev2gym_amd.engine import host_ars_update
    tag = "pst-linear"
    kind, D, h1, h2, P = ac.net_of(tag)
    case = ac.large_update(n_delta)
    theta, delta, lr = case["theta"], case["delta"], case["lr"]
    assert theta.size == 1260
    a = _create(eng, tag, -1.0, n_delta, theta, n_top=n_top, learning_rate=lr, delta_std=case["delta_std"])
    x = np.random.default_rng(8).normal(size=(33, D)).astype(np.float32)
    try:
        before = _act(eng, a, x, P, False)
        for kind_r in ac.LARGE_KINDS:
            returns = ac.large_returns(n_delta, n_top, kind_r)
            eng.ars_set_weights(a, theta)
            eng.ars_seed(a, ac.EDGE_SEED, 0)
            eng.ars_perturb(a)
            if kind_r == ac.LARGE_KINDS[0]:
                assert np.array_equal(_bits(eng.ars_get_deltas(a, n_delta, theta.size)), _bits(delta))
            eng.ars_set_returns(a, returns)
            eng.ars_update(a)
            rep = eng.ars_get_report(a, n_delta)
            new = eng.ars_get_weights(a, theta.size)
            want, wrep = host_ars_update(theta, delta, returns, n_top, lr)
            _record(f"ARS LARGE UPDATE n_delta {n_delta} n_top {n_top} {kind_r}: sigma_R {rep['sigma_r']:.6g} step {rep['step']:.6g} refused {rep['refused']} "
                    f"first_bad {rep['first_bad']}  theta bits differing from the twin {int((_bits(new) != _bits(want)).sum())}  ranks differing {int((rep['ranks'] != wrep['ranks']).sum())}")
            assert np.array_equal(_bits(new), _bits(want)) and np.array_equal(rep["ranks"], wrep["ranks"]) and np.array_equal(_bits(rep["returns"]), _bits(returns))
            assert _bits(np.float64(rep["sigma_r"])) == _bits(np.float64(wrep["sigma_r"])) and _bits(np.float64(rep["step"])) == _bits(np.float64(wrep["step"]))
            assert (rep["refused"], rep["first_bad"], rep["n_top"], rep["iteration"]) == (wrep["refused"], wrep["first_bad"], n_top, 0)
            after = _act(eng, a, x, P, False)
            if kind_r in ("nan", "inf"):
                assert rep["refused"] and rep["first_bad"] == (2 * n_delta - 1 if kind_r == "nan" else ac.LARGE_INF_AT)
                assert np.array_equal(_bits(new), _bits(theta)) and np.array_equal(_bits(after), _bits(before))
                continue
            assert np.array_equal(rep["ranks"], ac.stable_ranks(returns)) and sorted(rep["ranks"].tolist()) == list(range(n_delta))
            assert not rep["refused"] and rep["first_bad"] == -1 and (new != theta).any() and not np.array_equal(_bits(after), _bits(before))
            if kind_r == "distinct":
                ref, info = ars_update_numpy(theta, delta, returns, n_top, lr)
                tol = EPS32 * np.maximum(np.abs(ref), TINY32)
                err = np.abs(new.astype(np.float64) - ref)
                _record(f"ARS LARGE UPDATE n_delta {n_delta} n_top {n_top} distinct: |theta - f64| worst err/tol {(err / tol).max():.3f}  moved {np.abs(ref - theta).max():.3e}")
                assert (err <= tol).all() and np.array_equal(np.argsort(rep["ranks"])[:n_top], info["order"])
    finally:
        eng.ars_destroy(a)


# ---- rollouts with wide and with many candidates ----
def _pool_engine(n_envs):
    """_engine's pool at another width, whatever kernel it takes; (engine, the registered hand-over pair or None)"""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    _, batch, rk, sk = load_golden(os.path.join(GOLDEN_DIR, "pst_rand_s2.npz"))
    e = Engine(batch.tile(n_envs), rk, sk, device=0, flags=_abi.FLAG_LOG_SOC, n_active_envs=n_envs)
    assert (e.E, e.D, e.P) == (n_envs, 63, 20)
    return e


def _route(eng, a):
    """Registers the float32 hand-over pair where the shape does not take the direct route (ev2g_ars_rollout refuses, k_steps 0 steps nothing)"""
    from ev2gym_amd.engine import EngineError
    try:
        eng.ars_rollout(a, 0, population=False)
        return "direct", ()
    except EngineError as e:
        assert "hand-over" in str(e), e
    pair = (eng.empty((eng.E, eng.D), np.float32), eng.empty((eng.E, eng.P), np.float32))
    eng.set_extras(obs_f32=pair[0], actions_f32=pair[1])
    eng.ars_rollout(a, 0, population=False)
    return "registered hand-over pair", pair


@pytest.mark.parametrize("E,n_delta,check", [(132, 2, (0, 1, 2, 3)), (516, 129, (0, 128, 257))])
def test_population_episodes_with_wide_and_with_many_candidates(E, n_delta, check):
    from ev2gym_amd.engine import host_ars_returns
    tag, offset, seed = "pst-33-17", -0.5, 4
    kind, D, h1, h2, P = ac.net_of(tag)
    C, R = 2 * n_delta, E // (2 * n_delta)
    eng = _pool_engine(E)
    T = eng.T
    theta = ac.random_theta(tag)
    a = _create(eng, tag, 0.0, n_delta, theta, seed=seed, delta_std=0.3, alive_bonus_offset=offset)
    rew, rew_c = eng.empty((T, E)), eng.empty((T, E))
    others, pair = [], ()
    try:
        route, pair = _route(eng, a)
        _record(f"ARS WIDE ROLLOUT E {E} C {C} R {R}: kernel {eng.kernel_name}, {route}")
        eng.ars_perturb(a)
        eng.reset_f32(eng.ars_obs_f32(a), 0)
        eng.ars_rollout(a, T, population=True, reward=rew, r_stride=E)
        eng.synchronize()
        kept = rew.to_host()
        env = np.zeros(E)
        host_ars_returns(env, kept)
        want = host_ars_returns(env, None, C, offset, T)
        got_env = eng.ars_get_env_returns(a)
        eng.ars_update(a)
        rep = eng.ars_get_report(a, n_delta)
        _record(f"ARS WIDE ROLLOUT E {E} C {C} R {R}: max |reward| {np.abs(kept).max():.6g}  candidate returns {rep['returns'].min():.6g} .. {rep['returns'].max():.6g}  "
                f"env returns differing from the twin {int((_bits(got_env) != _bits(env)).sum())}  candidate returns differing {int((_bits(rep['returns']) != _bits(want)).sum())}")
        assert np.abs(kept).max() > 0 and np.isfinite(kept).all() and eng.current_step == T and eng.ars_counters(a)[2] == T
        assert np.array_equal(_bits(got_env), _bits(env))
        assert np.array_equal(_bits(rep["returns"]), _bits(want)) and len(set(rep["returns"].tolist())) > 1 and not rep["refused"]
        for c in check:   # the candidate's weights as a centre policy on the same window: its envs' rewards, whatever R, C and the rows' places
            b = _create(eng, tag, 0.0, 1, eng.ars_get_candidate(a, c, theta.size))
            others.append(b)
            eng.reset_f32(eng.ars_obs_f32(b), 0)
            eng.ars_rollout(b, T, population=False, reward=rew_c, r_stride=E)
            eng.synchronize()
            alone = rew_c.to_host()
            assert np.array_equal(_bits(alone[:, c * R:(c + 1) * R]), _bits(kept[:, c * R:(c + 1) * R])), c
            assert not np.array_equal(_bits(alone), _bits(kept)), c   # (the other candidates' envs ran under other weights)
    finally:
        eng.set_extras()
        for b in others + [a]:
            eng.ars_destroy(b)
        for buf in (rew, rew_c) + tuple(pair):
            buf.free()
        eng.close()


# ---- a centre rollout is no part of an iteration ----
@pytest.mark.parametrize("tag", ["pst-33-17", "pst-linear"])
def test_a_centre_episode_between_perturb_and_update_changes_nothing(eng, tag):
    kind, D, h1, h2, P = ac.net_of(tag)
    E, T, n_delta, seed = eng.E, eng.T, 2, 4
    theta = ac.random_theta(tag)
    rew = eng.empty((T, E))
    out = {}
    try:
        for how in ("plain", "with a centre episode"):
            a = _create(eng, tag, 0.0, n_delta, theta, seed=seed, delta_std=0.3, alive_bonus_offset=-0.5, learning_rate=0.02)
            try:
                eng.ars_perturb(a)
                centre = None
                if how != "plain":   # as ARSLearner.evaluate(): a whole episode of theta that keeps its own reward rows
                    eng.reset_f32(eng.ars_obs_f32(a), 0)
                    eng.ars_rollout(a, T, population=False, reward=rew, r_stride=E)
                    eng.synchronize()
                    centre = rew.to_host()
                    assert np.abs(centre).max() > 0 and eng.ars_counters(a)[2] == 0
                    assert not eng.ars_get_env_returns(a).any(), "a centre rollout must not add to the envs' returns"
                eng.reset_f32(eng.ars_obs_f32(a), 0)
                eng.ars_rollout(a, T, population=True)
                env = eng.ars_get_env_returns(a)
                steps = eng.ars_counters(a)[2]
                eng.ars_update(a)
                out[how] = (eng.ars_get_report(a, n_delta), eng.ars_get_weights(a, theta.size), env, steps)
            finally:
                eng.ars_destroy(a)
        (rep0, th0, env0, st0), (rep1, th1, env1, st1) = out["plain"], out["with a centre episode"]
        _record(f"ARS CENTRE CONTRACT {tag}: returns {rep0['returns']} against {rep1['returns']} with a centre episode; steps {st0} against {st1}")
        assert st0 == st1 == T and np.array_equal(_bits(env0), _bits(env1))
        assert np.array_equal(_bits(rep0["returns"]), _bits(rep1["returns"])) and np.array_equal(rep0["ranks"], rep1["ranks"])
        for k in ("sigma_r", "step"):
            assert _bits(np.float64(rep0[k])) == _bits(np.float64(rep1[k])), k
        for k in ("refused", "first_bad", "n_top", "iteration"):
            assert rep0[k] == rep1[k], k
        assert np.array_equal(_bits(th0), _bits(th1)) and (th0 != theta).any() and not rep0["refused"]
    finally:
        rew.free()


def _same_report(got, want):
    assert np.array_equal(_bits(got["returns"]), _bits(want["returns"])) and np.array_equal(got["ranks"], want["ranks"])
    for k in ("sigma_r", "step"):
        assert _bits(np.float64(got[k])) == _bits(np.float64(want[k])), k
    for k in ("refused", "first_bad", "n_top", "iteration"):
        assert got[k] == want[k], k


def test_evaluate_and_centre_segments_leave_trains_reports_unchanged():
    from ev2gym_amd.ars import ARSLearner
    n_delta, rounds = 2, 2
    eng = _engine(pool=3)
    E, M, T = eng.E, eng.M, eng.T
    kw = dict(policy="MlpPolicy", n_delta=n_delta, learning_rate=0.02, delta_std=0.05, alive_bonus_offset=0.25, n_eval_episodes=rounds * E // (2 * n_delta), seed=11,
              net_arch=(33, 17), lo=0.0)
    seg = eng.empty((T // 2, E))
    try:
        plain = ARSLearner(eng, **kw)
        assert plain.rounds == rounds
        start = eng.scenario_offset
        want = [plain.train(), plain.train()]
        theta = plain.get_weights()
        plain.close()
        eng.reset(offset=start)
        busy = ARSLearner(eng, **kw)
        # iteration 0 by hand, with a centre segment between its two rounds (on another window, which the next round's reset leaves behind)
        eng.ars_perturb(busy.ars)
        off = (start + E) % M
        busy._episode(True, off)
        eng.reset_f32(busy.obs32, (off + 5) % M)
        eng.ars_rollout(busy.ars, T // 2, population=False, reward=seg, r_stride=E)
        eng.synchronize()
        assert np.abs(seg.to_host()).max() > 0, "the centre segment must earn rewards, or adding them would change nothing"
        busy._episode(True, (off + E) % M)
        eng.ars_update(busy.ars)
        got0 = eng.ars_get_report(busy.ars, n_delta)
        after = eng.scenario_offset
        mean = busy.evaluate(1)   # a whole centre episode between two train() calls; it moves the window, so the next train() is told its own
        got1 = busy.train(first_offset=(after + E) % M)
        _record(f"ARS CENTRE CONTRACT learner: evaluate() {mean:.6g}; iteration 0 returns {got0['returns']} (plain {want[0]['returns']}); iteration 1 returns "
                f"{got1['returns']} (plain {want[1]['returns']})")
        assert np.isfinite(mean) and mean != 0.0
        _same_report(got0, want[0])
        _same_report(got1, want[1])
        assert np.array_equal(_bits(busy.get_weights()), _bits(theta)) and (theta != 0).any()
        busy.close()
    finally:
        seg.free()
        eng.close()


# ---- the rates act ----
def test_set_rates_changes_the_next_perturb_and_the_next_update(eng):
    from ev2gym_amd.engine import host_ars_perturb, host_ars_update
    tag, n_delta, n_top, seed, lr, std = "pst-33-17", 3, 2, 19, 0.02, 0.05
    theta = ac.random_theta(tag)
    returns = np.array([3.0, -1.0, 7.5, 2.0, 0.5, 4.0])
    a = _create(eng, tag, -1.0, n_delta, theta, seed=seed, n_top=n_top, learning_rate=lr, delta_std=std)
    try:
        eng.ars_perturb(a)
        old = np.stack([eng.ars_get_candidate(a, c, theta.size) for c in range(2 * n_delta)])
        old_delta = eng.ars_get_deltas(a, n_delta, theta.size)
        assert np.array_equal(_bits(old), _bits(host_ars_perturb(theta, n_delta, std, seed, 0)[1]))
        # delta_std doubled: the same draws, unscaled; candidates twice as far out
        eng.ars_set_rates(a, lr, 2 * std)
        eng.ars_seed(a, seed, 0)
        eng.ars_perturb(a)
        new = np.stack([eng.ars_get_candidate(a, c, theta.size) for c in range(2 * n_delta)])
        delta, cand = host_ars_perturb(theta, n_delta, 2 * std, seed, 0)
        assert np.array_equal(_bits(new), _bits(cand)) and (new != old).mean() > 0.9
        assert np.array_equal(_bits(eng.ars_get_deltas(a, n_delta, theta.size)), _bits(old_delta)) and np.array_equal(_bits(old_delta), _bits(delta))
        spread = np.abs(new.astype(np.float64) - theta).max() / np.abs(old.astype(np.float64) - theta).max()
        # learning rate halved: the twin's step and theta under the new rate, not under the old
        eng.ars_set_rates(a, lr / 2, 2 * std)
        eng.ars_set_returns(a, returns)
        eng.ars_update(a)
        rep, got = eng.ars_get_report(a, n_delta), eng.ars_get_weights(a, theta.size)
        want, wrep = host_ars_update(theta, delta, returns, n_top, lr / 2)
        full, frep = host_ars_update(theta, delta, returns, n_top, lr)
        _record(f"ARS RATES: candidates' spread x{spread:.4f} under 2 delta_std; step {rep['step']:.6g} under lr / 2 (twin {wrep['step']:.6g}; {frep['step']:.6g} under lr)")
        assert abs(spread - 2.0) < 1e-3
        assert _bits(np.float64(rep["step"])) == _bits(np.float64(wrep["step"])) and rep["step"] != frep["step"] and not rep["refused"]
        assert np.array_equal(_bits(got), _bits(want)) and not np.array_equal(_bits(got), _bits(full)) and (got != theta).any()
        # learning rate 0: a step of 0, theta keeps its bits, nothing is refused
        eng.ars_set_rates(a, 0.0, 2 * std)
        eng.ars_perturb(a)
        eng.ars_set_returns(a, returns)
        eng.ars_update(a)
        rep = eng.ars_get_report(a, n_delta)
        assert rep["step"] == 0.0 and not rep["refused"] and rep["first_bad"] == -1 and rep["iteration"] == 1
        assert np.array_equal(_bits(eng.ars_get_weights(a, theta.size)), _bits(got))
    finally:
        eng.ars_destroy(a)
