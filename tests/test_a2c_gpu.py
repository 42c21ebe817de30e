"""The A2C learner on the device (csrc/ev2g_ppo.h; ev2g_a2c_*; ev2gym_amd/a2c.py): the gradient of an update against the float64 reference for
all thirteen arrays and the statistics, bit-for-bit determinism, clip + RMSprop (and Adam) over consecutive updates against a float64 torch
loop, the repacked weight images against a fresh policy object, A2CLearner.train() end to end behind a collector, that the value loss falls,
and every refusal through the ABI.

Tolerance (the idiom of tests/test_ppo_gpu.py, helpers in tests/test_ppo_cpu.py and tests/test_a2c_cpu.py): reference = float64
(`a2c_update_numpy`, or the torch float64 loop); d32 = the largest deviation from it of the same computation in torch-CPU float32; the device
gets 4 d32 + 4 * 2^-23 * s with s = max(1, |y|) for parameters and statistics and the array's largest reference magnitude for gradients.
Every d32 and every device deviation is printed before it is asserted, and appended to the file EV2G_PPO_RECORD names.

Handles: the 37-env, 12-step generated PublicPST pool (D 63, P 20) and the v2gppl_rand_s2 fixture's engine; the D 162 / P 50 networks are
created with their shape spelled out, as tests/test_ppo_gpu.py does."""
import functools

import numpy as np
import pytest

from tests import learner_cases
from tests.learner_cases import N_ROWS, NAMES, SHAPES, _index_sets, _shape, engines  # noqa: F401 (engines: the fixture)
from tests.test_a2c_cpu import a2c_reference, a2c_torch_grads, a2c_torch_train
from tests.test_onpolicy_gpu import _bits, _gen_engine, _up
from tests.test_ppo_cpu import _record, grad_tol, make_case, value_tol

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
_Device = functools.partial(learner_cases._Device, "a2c")


def _compare_grads(tag, got, got_stats, ref, ref_stats, y32, y32_stats):
    ok = True
    for name, g, r, y in zip(NAMES, got, ref, y32):
        assert g.shape == r.shape, name
        d32, dev, tol = float(np.abs(y - r).max()), float(np.abs(g - r).max()), grad_tol(r, float(np.abs(y - r).max()))
        _record(f"A2C GRAD {tag} {name}: d32 {d32:.3e}  |device - f64| {dev:.3e}  tol {tol:.3e}  max|ref| {np.abs(r).max():.3e}")
        ok &= bool(np.isfinite(g).all() and dev <= tol)
    d32 = float(np.abs(y32_stats - ref_stats).max())
    dev, tol = np.abs(got_stats - ref_stats), value_tol(ref_stats, d32)
    _record(f"A2C GRAD {tag} stats: d32 {d32:.3e}  |device - f64| {dev.max():.3e}  tol {tol.min():.3e}")
    return ok and bool((dev <= tol).all()) and got_stats[4] == 0.0 and got_stats[5] == 0.0


GRAD_CASES = [
    ("pst-tanh", "pst", (64, 64), (64, 64), "tanh"),
    ("ppl-tanh", "ppl", (64, 64), (64, 64), "tanh"),
    ("pst-relu", "pst", (64, 64), (64, 64), "relu"),
    ("ppl-relu", "ppl", (64, 64), (64, 64), "relu"),
    ("pst-odd", "pst", (33, 17), (40, 64), "tanh"),
]


@pytest.mark.parametrize("tag,kind,h,v,activation", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_gradients_match_the_float64_reference(engines, tag, kind, h, v, activation):
    import torch
    from ev2gym_amd.engine import ppo_query
    eng, (D, P) = engines[kind], SHAPES[kind]
    n_rows = N_ROWS[activation]
    case = make_case(D, P, h=h, v=v, activation=activation, n_rows=n_rows)
    if activation == "relu":
        assert case["zmin"] >= 1e-5
    cap = ppo_query(*_shape(case))["grid_cap"]
    ok = True
    for normalize in (False, True):
        for ent_coef in (0.0, 0.01):
            cfg = dict(vf_coef=0.5, ent_coef=ent_coef, normalize_advantage=normalize)
            dev = _Device(eng, case, **cfg)
            try:
                for idx in _index_sets(cap, n_rows, normalize):
                    ref, ref_stats, _ = a2c_reference(case, idx, **cfg)
                    y32, y32_stats = a2c_torch_grads(case, idx, torch.float32, **cfg)
                    got, got_stats = dev.grad(idx)
                    ok &= _compare_grads(f"{tag} normalize {normalize} ent_coef {ent_coef} B {len(idx)}", got, got_stats, ref, ref_stats, y32, y32_stats)
            finally:
                dev.close()
    assert ok


def test_the_same_calls_give_the_same_bits(engines):
    from ev2gym_amd.engine import ppo_query
    eng, (D, P) = engines["ppl"], SHAPES["ppl"]
    case = make_case(D, P, n_rows=600)
    sets = _index_sets(ppo_query(*_shape(case))["grid_cap"], 600, True)
    runs = []
    for _ in range(2):   # two fresh learners, the same calls
        dev = _Device(eng, case, ent_coef=0.01, normalize_advantage=True)
        try:
            g1, s1 = dev.grad(sets[-1])
            g2, s2 = dev.grad(sets[-1])
            for name, a, b in zip(NAMES, g1, g2):
                assert np.array_equal(_bits(a), _bits(b)), name
            assert np.array_equal(_bits(s1), _bits(s2))
            stats = [dev.update(ix) for ix in (sets[-1], sets[3], sets[1])]
            last, _ = dev.grad(sets[0])
            runs.append((g1, stats, dev.weights(), last))
        finally:
            dev.close()
    (ga, sa, wa, la), (gb, sb, wb, lb) = runs
    for name, *pairs in zip(NAMES, ga, gb, wa, wb, la, lb):
        for a, b in zip(pairs[0::2], pairs[1::2]):
            assert np.array_equal(_bits(a), _bits(b)), name
    assert np.array_equal(_bits(np.array(sa)), _bits(np.array(sb)))
    assert any(not np.array_equal(w, w0) for w, w0 in zip(wa, case["weights"]))   # (the updates moved the weights)


def _compare_params(tag, got, ref, y32, start):
    """Parameters after the updates, and the optimiser's effect got - start against ref - start (the same deviation, set against how far
    the optimiser moved the array: an optimiser that did not run, or ran with another rate, shows up as a relative deviation near 1)."""
    ok = True
    for name, g, r, y, w0 in zip(NAMES, got, ref, y32, start):
        d32 = float(np.abs(y - r).max())
        dev, tol = np.abs(g.astype(np.float64) - r), value_tol(r, d32)
        moved = float(np.abs(r - np.asarray(w0, np.float64)).max())
        _record(f"A2C PARAM {tag} {name}: d32 {d32:.3e}  |device - f64| {dev.max():.3e}  tol {tol.min():.3e}  moved {moved:.3e}")
        ok &= bool(np.isfinite(g).all() and (dev <= tol).all())
        ok &= moved > 0.0 and float(np.abs((g.astype(np.float64) - w0) - (r - w0)).max()) <= float(tol.max())
    return ok


STEP_CASES = [("pst", "tanh", 0.5, True, True), ("ppl", "relu", 1.0e6, False, True), ("pst", "tanh", 0.5, True, False), ("ppl", "relu", 1.0e6, False, False)]


@pytest.mark.parametrize("kind,activation,max_grad_norm,binds,use_rms_prop", STEP_CASES,
                         ids=["rmsprop-clip-binds", "rmsprop-clip-idle", "adam-clip-binds", "adam-clip-idle"])
def test_three_updates_and_the_repacked_images(engines, kind, activation, max_grad_norm, binds, use_rms_prop):
    import torch
    from ev2gym_amd.onpolicy import GaussianActorCritic
    eng, (D, P) = engines[kind], SHAPES[kind]
    n_rows = N_ROWS[activation]
    case = make_case(D, P, activation=activation, n_rows=n_rows)
    rng = np.random.default_rng(21)
    sets = [rng.choice(n_rows, B, replace=False) for B in (64, 95, 33)]
    cfg = dict(vf_coef=0.5, ent_coef=0.01, normalize_advantage=(kind == "ppl"))
    loop = dict(max_grad_norm=max_grad_norm, use_rms_prop=use_rms_prop, **cfg)
    ref, ref_stats, norms = a2c_torch_train([case] * 3, sets, torch.float64, **loop)
    y32, y32_stats, _ = a2c_torch_train([case] * 3, sets, torch.float32, **loop)
    assert all((n > max_grad_norm) == binds for n in norms), norms
    dev = _Device(eng, case, **loop)
    fresh = None
    try:
        stats = np.array([dev.update(ix) for ix in sets])
        got = dev.weights()
        tag = f"{kind} {activation} {'RMSprop' if use_rms_prop else 'Adam'} max_grad_norm {max_grad_norm}"
        ok = _compare_params(tag, got, ref, y32, list(case["weights"]) + [case["log_std"]])
        d32 = float(np.abs(y32_stats - ref_stats).max())
        sdev = np.abs(stats - ref_stats)
        _record(f"A2C PARAM {tag} stats of the three updates: d32 {d32:.3e}  |device - f64| {sdev.max():.3e}  tol {value_tol(ref_stats, d32).min():.3e}")
        assert ok and (sdev <= value_tol(ref_stats, d32)).all()
        # the repacked images: a second policy object created from the read-back arrays computes the same bits
        fresh = GaussianActorCritic(got[:12], got[12], activation=activation, lo=-1.0, seed=5).attach(eng)
        x = np.concatenate([np.zeros((1, D), np.float32), case["obs"][:36]])   # (row 0: the all-zero observation)
        dx = _up(eng, x)
        out = [[eng.empty((37, P), np.float32), eng.empty((37,), np.float32)] for _ in range(2)]
        for ac, (m, v) in zip((dev.pol.ac, fresh.ac), out):
            eng.ac_forward(ac, dx, 37, mean=m, value=v)
        eng.synchronize()
        for a, b in zip(*out):
            assert np.array_equal(_bits(a.to_host()), _bits(b.to_host()))
        for b in [dx] + sum(out, []):
            b.free()
    finally:
        if fresh is not None:
            fresh.close()
        dev.close()


# ---- A2CLearner behind a collector ----
def _collected_case(pol, batch, weights, log_std):
    f = lambda t, *s: t.reshape(-1, *s).cpu().numpy()  # noqa: E731
    return dict(weights=weights, log_std=log_std, activation=pol.activation, obs=f(batch.observations, pol.d_in), actions=f(batch.actions, pol.d_out),
                advantages=f(batch.advantages), returns=f(batch.returns), values=f(batch.values))


def _explained_variance(values, returns, dtype):
    import torch
    v, r = torch.tensor(values, dtype=dtype), torch.tensor(returns, dtype=dtype)
    return float(1.0 - torch.var(r - v, unbiased=False) / torch.var(r, unbiased=False))


def test_train_end_to_end_behind_a_collector():
    import torch
    from ev2gym_amd.a2c import A2CLearner
    from ev2gym_amd.onpolicy import SB3_KEYS, SB3_LOG_STD, GaussianActorCritic, OnPolicyCollector, init_ac_weights
    eng = _gen_engine("pst", pool=3)
    w0, ls0 = init_ac_weights(eng.D, eng.P, seed=3), np.full(eng.P, -0.5, np.float32)
    pol = GaussianActorCritic(w0, ls0, lo=0.0, seed=5).attach(eng)
    fresh = None
    try:
        col = OnPolicyCollector(eng, pol, n_steps=5, gae_lambda=1.0)   # SB3's A2C defaults; 12-step episodes: the third rollout crosses an episode end
        learner = A2CLearner(col)
        cases, stats = [], []
        for _ in range(3):
            batch = col.collect().clone()
            stats.append(learner.train(batch))
            cases.append(_collected_case(pol, batch, w0, ls0))
        assert col.episodes >= 1
        N = 5 * eng.E
        sets = [np.arange(N)] * 3
        ref, ref_stats, _ = a2c_torch_train(cases, sets, torch.float64)
        y32, y32_stats, _ = a2c_torch_train(cases, sets, torch.float32)
        sd = learner.state_dict()
        got = [sd[k] for k in SB3_KEYS] + [sd[SB3_LOG_STD]]
        ok = _compare_params("END-TO-END", got, ref, y32, list(w0) + [ls0])
        gs = np.array([[s[k] for k in ("policy_loss", "value_loss", "entropy_loss", "loss")] for s in stats])
        d32 = float(np.abs(y32_stats - ref_stats).max())
        sdev, tol = np.abs(gs - ref_stats[:, :4]), value_tol(ref_stats[:, :4], d32)
        _record(f"A2C END-TO-END stats: d32 {d32:.3e}  |device - f64| {sdev.max():.3e}  tol {tol.min():.3e}")
        ok &= bool((sdev <= tol).all())
        for k, (c, s) in enumerate(zip(cases, stats)):
            e64, e32 = _explained_variance(c["values"], c["returns"], torch.float64), _explained_variance(c["values"], c["returns"], torch.float32)
            e_np = 1.0 - np.var(c["returns"].astype(np.float64) - c["values"]) / np.var(c["returns"].astype(np.float64))
            assert abs(e64 - e_np) <= 1e-12 * max(1.0, abs(e_np))
            d32, edev = abs(e32 - e_np), abs(s["explained_variance"] - e_np)
            _record(f"A2C END-TO-END explained_variance round {k}: numpy {e_np:.6e}  d32 {d32:.3e}  |device - f64| {edev:.3e}  "
                    f"tol {float(value_tol(np.array(e_np), d32)):.3e}")
            ok &= edev <= float(value_tol(np.array(e_np), d32))
        assert ok
        # afterwards the collector's policy samples exactly as a fresh one built from state_dict(), same seed and draw counter
        fresh = GaussianActorCritic(got[:12], got[12], lo=0.0, seed=5).attach(eng)
        dx = _up(eng, cases[2]["obs"][:37])
        acts = [[eng.empty((37, eng.P), np.float32), eng.empty((37, eng.P), np.float32), eng.empty((37,), np.float32)] for _ in range(2)]
        for ac, (a, c, lp) in zip((pol.ac, fresh.ac), acts):
            eng.ac_seed(ac, 11, 3)
            eng.ac_act(ac, dx, 37, actions=a, clipped=c, log_prob=lp)
        eng.synchronize()
        for a, b in zip(*acts):
            assert np.array_equal(_bits(a.to_host()), _bits(b.to_host()))
        # ... and the collector goes on with the new weights
        b2 = col.collect()
        v0 = torch.zeros(eng.E, dtype=torch.float32, device=b2.values.device)
        eng.ac_forward(pol.ac, b2.observations[0], eng.E, value=v0)
        eng.synchronize()
        assert np.array_equal(_bits(b2.values[0].cpu().numpy()), _bits(v0.cpu().numpy()))
        for b in [dx] + sum(acts, []):
            b.free()
    finally:
        if fresh is not None:
            fresh.close()
        pol.close()
        eng.close()


def test_value_loss_falls_over_200_updates(engines):
    """One fixed batch of 160 rows whose returns are a function of the observation (1.5 + a fixed linear form): something a value net can
    learn.  The last value loss is below half the first."""
    eng, (D, P) = engines["pst"], SHAPES["pst"]
    case = dict(make_case(D, P, n_rows=160))
    c = np.random.default_rng(4).normal(0.0, 1.0, D) / np.sqrt(D)
    case["returns"] = (1.5 + case["obs"].astype(np.float64) @ c).astype(np.float32)
    dev = _Device(eng, case, vf_coef=0.5)
    try:
        idx = np.arange(160)
        ix = _up(eng, idx.astype(np.int32))
        first = dev.update(idx)
        for _ in range(198):
            eng.a2c_update(dev.a2c, *dev.bufs, ix, 160)
        last = dev.update(idx)
        ix.free()
        _record(f"A2C SANITY value_loss of update 1 -> update 200 on one batch: {first[1]:.6e} -> {last[1]:.6e}")
        assert np.isfinite(last).all() and last[1] < 0.5 * first[1]
    finally:
        dev.close()


# ---- refusals ----
def test_refusals_through_the_abi(engines):
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.onpolicy import GaussianActorCritic, init_ac_weights
    eng = engines["pst"]
    case = make_case(eng.D, eng.P, n_rows=64)
    dev = _Device(eng, case)
    old_lp = _up(eng, np.zeros(64, np.float32))

    def refused(code, word, fn, *a, **kw):
        with pytest.raises(EngineError) as e:
            fn(*a, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)

    try:
        ix = _up(eng, np.arange(8, dtype=np.int32))
        refused(STATE, "no gradient", eng.a2c_apply, dev.a2c)
        for k in range(4):
            bufs = list(dev.bufs)
            bufs[k] = None
            refused(ARG, "null", eng.a2c_grad, dev.a2c, *bufs, ix, 8)
        refused(ARG, "null", eng.a2c_grad, dev.a2c, *dev.bufs, None, 8)
        refused(ARG, "null", eng.a2c_grad, None, *dev.bufs, ix, 8)
        refused(ARG, "null", eng.a2c_apply, None)
        refused(ARG, "B must be", eng.a2c_grad, dev.a2c, *dev.bufs, ix, 0)
        refused(ARG, "B must be", eng.a2c_update, dev.a2c, *dev.bufs, ix, -3)
        refused(ARG, "lr", eng.a2c_set_rate, dev.a2c, float("nan"))
        refused(ARG, "lr", eng.a2c_set_rate, dev.a2c, -1.0)
        # a second learner of either kind
        refused(STATE, "already has a learner", eng.a2c_create, dev.pol.ac)
        refused(STATE, "already has a learner", eng.ppo_create, dev.pol.ac)
        # PPO's entries on an A2C learner
        pb = (dev.bufs[0], dev.bufs[1], old_lp, dev.bufs[2], dev.bufs[3])
        refused(STATE, "A2C learner", eng.ppo_grad, dev.a2c, *pb, ix, 8)
        refused(STATE, "A2C learner", eng.ppo_minibatch, dev.a2c, *pb, ix, 8)
        refused(STATE, "A2C learner", eng.ppo_apply, dev.a2c)
        refused(STATE, "A2C learner", eng.ppo_set_rates, dev.a2c, 3e-4, 0.2)
        refused(STATE, "no gradient", eng.a2c_apply, dev.a2c)   # (nothing above left a gradient behind)
        # ... and A2C's entries on a PPO learner; a learner with normalisation refuses one row
        other = GaussianActorCritic(case["weights"], case["log_std"]).attach(eng)
        ppo = eng.ppo_create(other.ac)
        refused(STATE, "PPO learner", eng.a2c_grad, ppo, *dev.bufs, ix, 8)
        refused(STATE, "PPO learner", eng.a2c_update, ppo, *dev.bufs, ix, 8)
        refused(STATE, "PPO learner", eng.a2c_apply, ppo)
        refused(STATE, "PPO learner", eng.a2c_set_rate, ppo, 7e-4)
        refused(STATE, "already has a learner", eng.a2c_create, other.ac)
        eng.ppo_destroy(ppo)
        norm = eng.a2c_create(other.ac, normalize_advantage=True)   # (the destroyed learner freed the policy's slot)
        refused(ARG, "normalize_advantage", eng.a2c_grad, norm, *dev.bufs, ix, 1)
        refused(ARG, "normalize_advantage", eng.a2c_update, norm, *dev.bufs, ix, 1)
        eng.a2c_grad(norm, *dev.bufs, ix, 2)
        # destroying the policy destroys the learner
        other.close()
        refused(ARG, "not created on this handle", eng.a2c_apply, norm)
        # a foreign handle's policy and learner
        far = _gen_engine("pst")
        far_pol = GaussianActorCritic(case["weights"], case["log_std"]).attach(far)
        refused(ARG, "not created on this handle", eng.a2c_create, far_pol.ac)
        refused(ARG, "not created on this handle", far.a2c_apply, dev.a2c)
        far_pol.close()
        far.close()
        # a network the plan refuses; non-finite and out-of-range config values, the field named
        wide = GaussianActorCritic(init_ac_weights(eng.D, eng.P, h=(256, 256), v=(256, 256)), case["log_std"]).attach(eng)
        refused(ARG, "256 is too wide", eng.a2c_create, wide.ac)
        for kw, word in ((dict(lr=float("inf")), "lr"), (dict(lr=-1e-3), "lr"), (dict(alpha=1.0), "alpha"), (dict(alpha=float("nan")), "alpha"),
                         (dict(rms_eps=0.0), "rms_eps"), (dict(rms_eps=float("inf")), "rms_eps"), (dict(vf_coef=-1.0), "vf_coef"),
                         (dict(ent_coef=float("inf")), "ent_coef"), (dict(max_grad_norm=0.0), "max_grad_norm"),
                         (dict(max_grad_norm=float("nan")), "max_grad_norm")):
            refused(ARG, word, eng.a2c_create, wide.ac, **kw)
        wide.close()
        # the learner is as it was: a gradient, an apply, and the state error again
        eng.a2c_grad(dev.a2c, *dev.bufs, ix, 8)
        eng.a2c_apply(dev.a2c)
        refused(STATE, "no gradient", eng.a2c_apply, dev.a2c)
        eng.synchronize()
        ix.free()
    finally:
        old_lp.free()
        dev.close()
