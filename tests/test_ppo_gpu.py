"""The PPO learner on the device (csrc/ev2g_ppo.h; ev2g_ppo_*, ev2g_ac_get_weights; ev2gym_amd/ppo.py): the gradient of a minibatch against
the float64 reference for all thirteen arrays and the six statistics, bit-for-bit determinism, clip + Adam over consecutive minibatches against
a float64 torch loop, the repacked weight images against a fresh policy object, PPOLearner.train() end to end behind a collector, and every
refusal through the ABI.

Tolerance (the idiom of tests/test_onpolicy_gpu.py, helpers in tests/test_ppo_cpu.py): reference = float64 (`ppo_minibatch_numpy`, or the torch
float64 loop); d32 = the largest deviation from it of the same computation in torch-CPU float32; the device gets 4 d32 + 4 * 2^-23 * s with
s = max(1, |y|) for parameters and statistics and the array's largest reference magnitude for gradients (sums over the batch).  Every d32 and
every device deviation is printed before it is asserted, and appended to the file EV2G_PPO_RECORD names.

Handles: the 37-env, 12-step generated PublicPST pool (D 63, P 20) and the v2gppl_rand_s2 fixture's engine.  Networks: the two shipped shapes, D 63 /
P 20 and D 162 / P 50 (the fixture's own env is a smaller one, D 112 / P 25, so the D 162 / P 50 networks are created with their shape spelled
out: the learner's calls read caller arrays and need no env of that width).  Gradient rows are random observations in [0, 1] and random actions,
constructed away from the clip's and the ReLU's branches (tests/test_ppo_cpu.py's docstring)."""
import functools

import numpy as np
import pytest

from tests import learner_cases
from tests.learner_cases import N_ROWS, NAMES, SHAPES, _index_sets, _shape, engines  # noqa: F401 (engines: the fixture)
from tests.test_onpolicy_gpu import _bits, _gen_engine, _up
from tests.test_ppo_cpu import _record, check_branches, grad_tol, make_case, reference, torch_grads, torch_train, value_tol

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
_Device = functools.partial(learner_cases._Device, "ppo")


def _compare_grads(tag, got, got_stats, ref, ref_stats, y32, y32_stats):
    ok = True
    for name, g, r, y in zip(NAMES, got, ref, y32):
        assert g.shape == r.shape, name
        d32, dev, tol = float(np.abs(y - r).max()), float(np.abs(g - r).max()), grad_tol(r, float(np.abs(y - r).max()))
        _record(f"GRAD {tag} {name}: d32 {d32:.3e}  |device - f64| {dev:.3e}  tol {tol:.3e}  max|ref| {np.abs(r).max():.3e}")
        ok &= np.isfinite(g).all() and dev <= tol
    d32 = float(np.abs(y32_stats - ref_stats).max())
    dev, tol = np.abs(got_stats - ref_stats), value_tol(ref_stats, d32)
    _record(f"GRAD {tag} stats: d32 {d32:.3e}  |device - f64| {dev.max():.3e}  tol {tol.min():.3e}")
    return ok and bool((dev <= tol).all())


GRAD_CASES = [
    ("pst-tanh", "pst", (64, 64), (64, 64), "tanh", True, 0.0),
    ("ppl-tanh", "ppl", (64, 64), (64, 64), "tanh", True, 0.0),
    ("pst-relu", "pst", (64, 64), (64, 64), "relu", False, 0.0),
    ("ppl-relu-ent", "ppl", (64, 64), (64, 64), "relu", True, 0.01),
    ("pst-odd", "pst", (33, 17), (40, 64), "tanh", False, 0.0),
]


@pytest.mark.parametrize("tag,kind,h,v,activation,normalize,ent_coef", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_gradients_match_the_float64_reference(engines, tag, kind, h, v, activation, normalize, ent_coef):
    import torch
    from ev2gym_amd.engine import ppo_query
    eng, (D, P) = engines[kind], SHAPES[kind]
    n_rows = N_ROWS[activation]
    case = make_case(D, P, h=h, v=v, activation=activation, n_rows=n_rows)
    if activation == "relu":
        assert case["zmin"] >= 1e-5
    cfg = dict(vf_coef=0.5, ent_coef=ent_coef, normalize_advantage=normalize)
    dev = _Device(eng, case, **cfg)
    ok = True
    try:
        for idx in _index_sets(ppo_query(*_shape(case))["grid_cap"], n_rows):
            ref, ref_stats, aux = reference(case, idx, **cfg)
            if len(idx) >= 31:
                check_branches(aux)
            y32, y32_stats = torch_grads(case, idx, torch.float32, **cfg)
            got, got_stats = dev.grad(idx)
            ok &= _compare_grads(f"{tag} B {len(idx)}", got, got_stats, ref, ref_stats, y32, y32_stats)
        assert ok
    finally:
        dev.close()


def test_the_same_call_gives_the_same_bits(engines):
    from ev2gym_amd.engine import ppo_query
    eng, (D, P) = engines["ppl"], SHAPES["ppl"]
    case = make_case(D, P, n_rows=600)
    dev = _Device(eng, case, ent_coef=0.01)
    try:
        idx = _index_sets(ppo_query(*_shape(case))["grid_cap"], 600)[-1]
        g1, s1 = dev.grad(idx)
        g2, s2 = dev.grad(idx)
        for name, a, b in zip(NAMES, g1, g2):
            assert np.array_equal(_bits(a), _bits(b)), name
        assert np.array_equal(_bits(s1), _bits(s2))
    finally:
        dev.close()


def _compare_params(tag, got, ref, y32):
    ok = True
    for name, g, r, y in zip(NAMES, got, ref, y32):
        d32 = float(np.abs(y - r).max())
        dev, tol = np.abs(g.astype(np.float64) - r), value_tol(r, d32)
        _record(f"PARAM {tag} {name}: d32 {d32:.3e}  |device - f64| {dev.max():.3e}  tol {tol.min():.3e}")
        ok &= bool(np.isfinite(g).all() and (dev <= tol).all())
    return ok


@pytest.mark.parametrize("kind,activation,max_grad_norm,binds", [("pst", "tanh", 0.05, True), ("ppl", "relu", 1.0e3, False)],
                         ids=["clip-binds", "clip-idle"])
def test_three_minibatch_steps_and_the_repacked_images(engines, kind, activation, max_grad_norm, binds):
    import torch
    from ev2gym_amd.onpolicy import GaussianActorCritic
    eng, (D, P) = engines[kind], SHAPES[kind]
    n_rows = N_ROWS[activation]
    case = make_case(D, P, activation=activation, n_rows=n_rows)
    rng = np.random.default_rng(21)
    minibatches = [rng.choice(n_rows, B, replace=False) for B in (64, 95, 33)]
    cfg = dict(vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
    ref, ref_stats, norms = torch_train(case, minibatches, torch.float64, max_grad_norm=max_grad_norm, **cfg)
    y32, y32_stats, _ = torch_train(case, minibatches, torch.float32, max_grad_norm=max_grad_norm, **cfg)
    assert all((n > max_grad_norm) == binds for n in norms), norms
    dev = _Device(eng, case, max_grad_norm=max_grad_norm, **cfg)
    fresh = None
    try:
        stats = np.array([dev.minibatch(ix) for ix in minibatches])
        got = dev.weights()
        ok = _compare_params(f"{kind} {activation} max_grad_norm {max_grad_norm}", got, ref, y32)
        d32 = float(np.abs(y32_stats - ref_stats).max())
        sdev = np.abs(stats - ref_stats)
        _record(f"PARAM {kind} stats of the three steps: d32 {d32:.3e}  |device - f64| {sdev.max():.3e}  tol {value_tol(ref_stats, d32).min():.3e}")
        assert ok and (sdev <= value_tol(ref_stats, d32)).all()
        # the repacked images: a second policy object created from the read-back arrays computes the same bits ...
        fresh = GaussianActorCritic(got[:12], got[12], activation=activation, lo=-1.0, seed=5).attach(eng)
        x = np.concatenate([np.zeros((1, D), np.float32), case["obs"][:36]])   # (row 0: the all-zero observation)
        dx = _up(eng, x)
        out = [[eng.empty((37, P), np.float32), eng.empty((37,), np.float32)] for _ in range(2)]
        for ac, (m, v) in zip((dev.pol.ac, fresh.ac), out):
            eng.ac_forward(ac, dx, 37, mean=m, value=v)
        eng.synchronize()
        assert np.array_equal(_bits(out[0][0].to_host()), _bits(out[1][0].to_host())) and np.array_equal(_bits(out[0][1].to_host()), _bits(out[1][1].to_host()))
        # ... and after the sync it samples the same actions, clipped actions and log-probabilities from the same draws
        eng.ppo_sync(dev.ppo)
        acts = [[eng.empty((37, P), np.float32), eng.empty((37, P), np.float32), eng.empty((37,), np.float32)] for _ in range(2)]
        for ac, (a, c, lp) in zip((dev.pol.ac, fresh.ac), acts):
            eng.ac_seed(ac, 11, 3)
            eng.ac_act(ac, dx, 37, actions=a, clipped=c, log_prob=lp)
        eng.synchronize()
        for a, b in zip(*acts):
            assert np.array_equal(_bits(a.to_host()), _bits(b.to_host()))
        assert not np.array_equal(acts[0][0].to_host(), out[0][0].to_host())   # (it did sample)
        for b in [dx] + sum(out, []) + sum(acts, []):
            b.free()
    finally:
        if fresh is not None:
            fresh.close()
        dev.close()


def test_padding_survives_the_repack(engines):
    """Unequal trunks with padding columns (33, 17) / (40, 64) on D 63 (the input padding column 63 included): after an apply the policy object
    still computes, bit for bit, what a fresh object packed on the host from the read-back masters computes -- on the all-zero observation
    (biases and padding only) and on rows with large entries, which a non-zero padding weight or bias would show up in."""
    from ev2gym_amd.onpolicy import GaussianActorCritic
    eng = engines["pst"]
    case = make_case(eng.D, eng.P, h=(33, 17), v=(40, 64), n_rows=600)
    dev = _Device(eng, case)
    fresh = None
    try:
        dev.minibatch(np.arange(50))
        got = dev.weights()
        fresh = GaussianActorCritic(got[:12], got[12], activation="tanh", lo=-1.0, seed=5).attach(eng)
        x = np.concatenate([np.zeros((1, eng.D), np.float32), 50.0 * case["obs"][:40]])
        dx = _up(eng, x)
        out = [[eng.empty((41, eng.P), np.float32), eng.empty((41,), np.float32)] for _ in range(2)]
        for ac, (m, v) in zip((dev.pol.ac, fresh.ac), out):
            eng.ac_forward(ac, dx, 41, mean=m, value=v)
        eng.synchronize()
        for a, b in zip(*out):
            assert np.array_equal(_bits(a.to_host()), _bits(b.to_host()))
        assert any(not np.array_equal(g, w) for g, w in zip(got, case["weights"]))   # (the step moved the weights)
        for b in [dx] + sum(out, []):
            b.free()
    finally:
        if fresh is not None:
            fresh.close()
        dev.close()


# ---- PPOLearner behind a collector ----
def _collected_case(pol, batch, weights, log_std):
    f = lambda t, *s: t.reshape(-1, *s).cpu().numpy()  # noqa: E731
    return dict(weights=weights, log_std=log_std, activation=pol.activation, obs=f(batch.observations, pol.d_in), actions=f(batch.actions, pol.d_out),
                old_log_prob=f(batch.log_probs), advantages=f(batch.advantages), returns=f(batch.returns))


def test_train_end_to_end_behind_a_collector():
    import torch
    from ev2gym_amd.onpolicy import GaussianActorCritic, OnPolicyCollector, init_ac_weights
    from ev2gym_amd.ppo import PPOLearner
    eng = _gen_engine("pst", pool=3)
    w0, ls0 = init_ac_weights(eng.D, eng.P, seed=3), np.full(eng.P, -0.5, np.float32)
    pol = GaussianActorCritic(w0, ls0, lo=0.0, seed=5).attach(eng)
    try:
        col = OnPolicyCollector(eng, pol, 24)   # 12-step episodes: an episode end falls inside the rollout
        batch = col.collect().clone()
        assert col.episodes >= 1
        N = 24 * eng.E
        rng = np.random.default_rng(2)
        minibatches = [p[i:i + 64] for p in (rng.permutation(N), rng.permutation(N)) for i in range(0, N, 64)]
        assert len(minibatches[-1]) == N % 64 != 0
        learner = PPOLearner(col, n_epochs=2, batch_size=64)
        stats = learner.train(batch, minibatches=minibatches)
        case = _collected_case(pol, batch, w0, ls0)
        ref, ref_stats, _ = torch_train(case, minibatches, torch.float64)
        y32, y32_stats, _ = torch_train(case, minibatches, torch.float32)
        sd = learner.state_dict()
        from ev2gym_amd.onpolicy import SB3_KEYS, SB3_LOG_STD
        got = [sd[k] for k in SB3_KEYS] + [sd[SB3_LOG_STD]]
        ok = _compare_params("END-TO-END", got, ref, y32)
        rs, ys = ref_stats.mean(axis=0), y32_stats.mean(axis=0)
        gs = np.array([stats[k] for k in ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction")])
        d32 = float(np.abs(ys - rs).max())
        _record(f"END-TO-END stats: d32 {d32:.3e}  |device - f64| {np.abs(gs - rs).max():.3e}  tol {value_tol(rs, d32).min():.3e}")
        assert ok and (np.abs(gs - rs) <= value_tol(rs, d32)).all()
        # the collector goes on with the new weights
        b2 = col.collect()
        v0 = torch.zeros(eng.E, dtype=torch.float32, device=b2.values.device)
        eng.ac_forward(pol.ac, b2.observations[0], eng.E, value=v0)
        eng.synchronize()
        assert np.array_equal(_bits(b2.values[0].cpu().numpy()), _bits(v0.cpu().numpy()))
        assert not np.array_equal(b2.values[0].cpu().numpy(), batch.values[0].cpu().numpy())
    finally:
        pol.close()
        eng.close()


def test_value_loss_falls_over_thirty_epochs():
    import torch
    from ev2gym_amd.onpolicy import GaussianActorCritic, OnPolicyCollector, init_ac_weights
    from ev2gym_amd.ppo import PPOLearner
    eng = _gen_engine("pst", pool=3)
    w0, ls0 = init_ac_weights(eng.D, eng.P, seed=4), np.full(eng.P, -0.5, np.float32)
    pol = GaussianActorCritic(w0, ls0, lo=0.0, seed=6).attach(eng)
    try:
        col = OnPolicyCollector(eng, pol, 24)
        batch = col.collect().clone()
        N, per = 24 * eng.E, 4
        rng = np.random.default_rng(3)
        minibatches = [p for _ in range(30) for p in np.array_split(rng.permutation(N), per)]
        learner = PPOLearner(col, n_epochs=30, batch_size=N // per)
        learner.train(batch, minibatches=minibatches)
        vl = learner.last_stats[:, 1].reshape(30, per).mean(axis=1)
        _, ref_stats, _ = torch_train(_collected_case(pol, batch, w0, ls0), minibatches, torch.float64)
        rl = ref_stats[:, 1].reshape(30, per).mean(axis=1)
        _record(f"SANITY value_loss first -> last epoch: device {vl[0]:.6e} -> {vl[-1]:.6e}, float64 loop {rl[0]:.6e} -> {rl[-1]:.6e}")
        assert vl[-1] < vl[0] and rl[-1] < rl[0]
    finally:
        pol.close()
        eng.close()


# ---- refusals ----
def test_refusals_through_the_abi(engines):
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.onpolicy import GaussianActorCritic, init_ac_weights
    eng = engines["pst"]
    case = make_case(eng.D, eng.P, n_rows=64)
    dev = _Device(eng, case)

    def refused(code, word, fn, *a, **kw):
        with pytest.raises(EngineError) as e:
            fn(*a, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)

    try:
        ix = _up(eng, np.arange(8, dtype=np.int32))
        refused(STATE, "no gradient", eng.ppo_apply, dev.ppo)
        for k in range(5):
            bufs = list(dev.bufs)
            bufs[k] = None
            refused(ARG, "null", eng.ppo_grad, dev.ppo, *bufs, ix, 8)
        refused(ARG, "null", eng.ppo_grad, dev.ppo, *dev.bufs, None, 8)
        refused(ARG, "null", eng.ppo_grad, None, *dev.bufs, ix, 8)
        refused(ARG, "B must be", eng.ppo_grad, dev.ppo, *dev.bufs, ix, 0)
        refused(ARG, "B must be", eng.ppo_minibatch, dev.ppo, *dev.bufs, ix, -3)
        refused(STATE, "already has a learner", eng.ppo_create, dev.pol.ac)
        refused(ARG, "lr", eng.ppo_set_rates, dev.ppo, float("nan"), 0.2)
        refused(ARG, "clip_range", eng.ppo_set_rates, dev.ppo, 3e-4, 0.0)
        refused(STATE, "no gradient", eng.ppo_apply, dev.ppo)   # (nothing above left a gradient behind)
        # a learner on a foreign handle's policy, and a foreign handle's learner
        far = _gen_engine("pst")
        far_pol = GaussianActorCritic(case["weights"], case["log_std"]).attach(far)
        refused(ARG, "not created on this handle", eng.ppo_create, far_pol.ac)
        refused(ARG, "not created on this handle", far.ppo_apply, dev.ppo)
        far_pol.close()
        far.close()
        # a network the plan refuses; non-finite and out-of-range config values
        wide = GaussianActorCritic(init_ac_weights(eng.D, eng.P, h=(256, 256), v=(256, 256)), case["log_std"]).attach(eng)
        refused(ARG, "256 is too wide", eng.ppo_create, wide.ac)
        for kw, word in ((dict(lr=float("inf")), "lr"), (dict(beta1=1.0), "beta1"), (dict(beta2=float("nan")), "beta2"), (dict(adam_eps=0.0), "adam_eps"),
                         (dict(clip_range=float("nan")), "clip_range"), (dict(vf_coef=-1.0), "vf_coef"), (dict(ent_coef=float("inf")), "ent_coef"),
                         (dict(max_grad_norm=0.0), "max_grad_norm")):
            refused(ARG, word, eng.ppo_create, wide.ac, **kw)
        wide.close()
        # the learner is as it was: a gradient, an apply, and the state error again
        eng.ppo_grad(dev.ppo, *dev.bufs, ix, 8)
        eng.ppo_apply(dev.ppo)
        refused(STATE, "no gradient", eng.ppo_apply, dev.ppo)
        eng.synchronize()
        ix.free()
    finally:
        dev.close()
