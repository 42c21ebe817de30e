"""The PPO and A2C learners on the device (csrc/ev2g_ppo.h) on every kind of network the plan accepts, and the effect of the rate setters.

tests/test_ppo_gpu.py and tests/test_a2c_gpu.py run learners whose layers all pad to 64: at most four tiles per stage for the gradient kernel's
four wavefronts, back tiles of depth 8, two tiles per image row.  The networks of tests/learner_cases.py's LEARNER_NETS take the same kernels
through a wavefront's second trip, deeper and shallower tiles, more tiles per image row, the LDS plan at its limit, one port, 64 ports, and
inputs and ports one past a tile (the table's comment says which row reaches what; tests/test_ppo_plan_cpu.py pins its LDS figures).  For each:
the thirteen gradients and the six statistics of PPO and A2C against the float64 reference over every index set of `_index_sets`; three optimiser
steps against the float64 torch loop, then the repacked images against a fresh policy object built from the read-back arrays (forward bits on the
all-zero observation, ordinary rows and 50x rows; sampled actions and log-probabilities after the sync); the same call twice for the same bits.

The rate setters (ev2g_ppo_set_rates, ev2g_a2c_set_rate, PPOLearner.set_rates, A2CLearner.set_rate): a gradient at clip 0.2, the setter, the
gradient again -- the second must be the float64 reference's at the new clip, which is asserted beforehand to differ from the old one by a
thousand tolerances; three steps with a different rate before each against the torch loop whose param group's lr is set likewise, where a
learner that kept its create-time rate is off by about the step size (the "moved" check sets the deviation against how far the optimiser went).

Tolerance: the project's (tests/test_ppo_gpu.py's docstring; grad_tol / value_tol of tests/test_ppo_cpu.py): reference = float64, d32 = the
deviation of torch-CPU float32 on the same rows, the device gets 4 d32 + 4 * 2^-23 * s.  Every figure is printed before it is asserted, and
appended to the file EV2G_PPO_RECORD names.

All networks run on one generated 37-env PublicPST engine: the learner's calls read caller arrays, so a policy is created with its shape spelled
out and needs no env of that width."""
import numpy as np
import pytest

from tests import learner_cases
from tests.learner_cases import LEARNER_NETS, N_ROWS, NAMES, _index_sets, _shape, net_shape
from tests.test_a2c_cpu import a2c_reference, a2c_torch_grads, a2c_torch_train
from tests.test_onpolicy_gpu import _bits, _gen_engine, _up
from tests.test_ppo_cpu import CLIP, _record, check_branches, grad_tol, make_case, reference, torch_grads, torch_train, value_tol

pytestmark = pytest.mark.gpu

NET_CASES = [(tag, act) for tag, row in LEARNER_NETS.items() for act in row[4]]
_ids = lambda cases: [f"{tag}-{act}" for tag, act, *_ in cases]  # noqa: E731


@pytest.fixture(scope="module")
def eng():
    e = _gen_engine("pst")
    yield e
    e.close()


_CASES = {}


def _net_case(tag, activation):
    """The rows of a network of the table (made once per module run; nothing changes them)."""
    if (tag, activation) not in _CASES:
        d_in, h, v, d_out, activations, _ = LEARNER_NETS[tag]
        assert activation in activations
        case = make_case(d_in, d_out, h=h, v=v, activation=activation, n_rows=N_ROWS[activation])
        assert activation == "tanh" or case["zmin"] >= 1e-5
        assert _shape(case) == net_shape(tag)
        _CASES[(tag, activation)] = case
    return _CASES[(tag, activation)]


def _grid_cap(case):
    from ev2gym_amd.engine import ppo_query
    return ppo_query(*_shape(case))["grid_cap"]   # (a network the plan refuses raises here: no row is skipped)


def _compare_grads(tag, got, got_stats, ref, ref_stats, y32, y32_stats):
    ok = True
    for name, g, r, y in zip(NAMES, got, ref, y32):
        assert g.shape == r.shape, name
        d32, dev, tol = float(np.abs(y - r).max()), float(np.abs(g - r).max()), grad_tol(r, float(np.abs(y - r).max()))
        _record(f"SHAPES GRAD {tag} {name}: d32 {d32:.3e}  |device - f64| {dev:.3e}  tol {tol:.3e}  max|ref| {np.abs(r).max():.3e}")
        ok &= bool(np.isfinite(g).all() and dev <= tol)
    d32 = float(np.abs(y32_stats - ref_stats).max())
    dev, tol = np.abs(got_stats - ref_stats), value_tol(ref_stats, d32)
    _record(f"SHAPES GRAD {tag} stats: d32 {d32:.3e}  |device - f64| {dev.max():.3e}  tol {tol.min():.3e}")
    return ok and bool((dev <= tol).all())


def _compare_params(tag, got, ref, y32, start):
    """Parameters after the steps, and the optimiser's effect got - start against ref - start (tests/test_a2c_gpu.py's check: an optimiser
    that ran with another rate shows up as a deviation near the distance moved)."""
    ok = True
    for name, g, r, y, w0 in zip(NAMES, got, ref, y32, start):
        d32 = float(np.abs(y - r).max())
        dev, tol = np.abs(g.astype(np.float64) - r), value_tol(r, d32)
        moved = float(np.abs(r - np.asarray(w0, np.float64)).max())
        _record(f"SHAPES PARAM {tag} {name}: d32 {d32:.3e}  |device - f64| {dev.max():.3e}  tol {tol.min():.3e}  moved {moved:.3e}")
        ok &= bool(np.isfinite(g).all() and (dev <= tol).all())
        ok &= moved > 0.0 and float(np.abs((g.astype(np.float64) - w0) - (r - w0)).max()) <= float(tol.max())
    return ok


def _compare_step_stats(tag, stats, ref_stats, y32_stats):
    d32 = float(np.abs(y32_stats - ref_stats).max())
    sdev, tol = np.abs(stats - ref_stats), value_tol(ref_stats, d32)
    _record(f"SHAPES PARAM {tag} stats of the steps: d32 {d32:.3e}  |device - f64| {sdev.max():.3e}  tol {tol.min():.3e}")
    return bool((sdev <= tol).all())


def _start(case):
    return list(case["weights"]) + [case["log_std"]]


# ---- gradients ----
@pytest.mark.parametrize("tag,activation", NET_CASES, ids=_ids(NET_CASES))
def test_ppo_gradients_match_the_float64_reference(eng, tag, activation):
    import torch
    case = _net_case(tag, activation)
    cfg = dict(vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
    dev = learner_cases._Device("ppo", eng, case, **cfg)
    ok = True
    try:
        sets = _index_sets(_grid_cap(case), N_ROWS[activation])
        assert [len(ix) for ix in sets[:5]] == [1, 31, 32, 33, 97] and len(sets[5]) > 32 * _grid_cap(case)
        for idx in sets:
            ref, ref_stats, aux = reference(case, idx, **cfg)
            if len(idx) >= 31:
                check_branches(aux)
            y32, y32_stats = torch_grads(case, idx, torch.float32, **cfg)
            got, got_stats = dev.grad(idx)
            ok &= _compare_grads(f"ppo {tag} {activation} B {len(idx)}", got, got_stats, ref, ref_stats, y32, y32_stats)
        assert ok
    finally:
        dev.close()


A2C_CASES = [(tag, act) for tag, act in NET_CASES if tag in ("wide", "limits", "tiny")]


@pytest.mark.parametrize("tag,activation", A2C_CASES, ids=_ids(A2C_CASES))
def test_a2c_gradients_match_the_float64_reference(eng, tag, activation):
    import torch
    case = _net_case(tag, activation)
    cfg = dict(vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
    dev = learner_cases._Device("a2c", eng, case, **cfg)
    ok = True
    try:
        for idx in _index_sets(_grid_cap(case), N_ROWS[activation], skip_one_row=True):
            ref, ref_stats, _ = a2c_reference(case, idx, **cfg)
            y32, y32_stats = a2c_torch_grads(case, idx, torch.float32, **cfg)
            got, got_stats = dev.grad(idx)
            ok &= _compare_grads(f"a2c {tag} {activation} B {len(idx)}", got, got_stats, ref, ref_stats, y32, y32_stats)
            ok &= bool(got_stats[4] == 0.0 and got_stats[5] == 0.0)   # the two ratio statistics: exact zeros
        assert ok
    finally:
        dev.close()


def test_the_same_call_gives_the_same_bits(eng):
    case = _net_case("wide", "tanh")
    dev = learner_cases._Device("ppo", eng, case, ent_coef=0.01)
    try:
        idx = _index_sets(_grid_cap(case), N_ROWS["tanh"])[-1]
        g1, s1 = dev.grad(idx)
        g2, s2 = dev.grad(idx)
        for name, a, b in zip(NAMES, g1, g2):
            assert np.array_equal(_bits(a), _bits(b)), name
        assert np.array_equal(_bits(s1), _bits(s2))
        assert all(np.abs(g).max() > 0.0 for g in g1)
    finally:
        dev.close()


# ---- three steps and the repacked images ----
# (tag, activation, learner, max_grad_norm, whether clip_grad_norm_ binds at every step or at none: asserted on the float64 loop's norms)
STEP_CASES = [
    ("wide", "tanh", "ppo", 0.05, True),
    ("limits", "relu", "ppo", 1.0e3, False),
    ("tiny", "tanh", "ppo", 0.5, False),
    ("lopsided", "relu", "a2c", 0.5, True),
]


@pytest.mark.parametrize("tag,activation,kind,max_grad_norm,binds", STEP_CASES, ids=[f"{c[0]}-{c[2]}" for c in STEP_CASES])
def test_three_steps_and_the_repacked_images(eng, tag, activation, kind, max_grad_norm, binds):
    import torch
    from ev2gym_amd.onpolicy import GaussianActorCritic
    case = _net_case(tag, activation)
    D, P, n_rows = case["D"], case["P"], N_ROWS[activation]
    rng = np.random.default_rng(21)
    sets = [rng.choice(n_rows, B, replace=False) for B in (64, 95, 33)]
    cfg = dict(vf_coef=0.5, ent_coef=0.01, normalize_advantage=True, max_grad_norm=max_grad_norm)
    if kind == "ppo":
        ref, ref_stats, norms = torch_train(case, sets, torch.float64, **cfg)
        y32, y32_stats, _ = torch_train(case, sets, torch.float32, **cfg)
    else:
        ref, ref_stats, norms = a2c_torch_train([case] * 3, sets, torch.float64, **cfg)
        y32, y32_stats, _ = a2c_torch_train([case] * 3, sets, torch.float32, **cfg)
    _record(f"SHAPES PARAM {kind} {tag} {activation} max_grad_norm {max_grad_norm}: the reference's gradient norms {['%.4e' % n for n in norms]}")
    assert all((n > max_grad_norm) == binds for n in norms), norms
    dev = learner_cases._Device(kind, eng, case, **cfg)
    fresh = None
    try:
        stats = np.array([dev.step(ix) for ix in sets])
        got = dev.weights()
        label = f"{kind} {tag} {activation} max_grad_norm {max_grad_norm}"
        ok = _compare_params(label, got, ref, y32, _start(case))
        ok &= _compare_step_stats(label, stats, ref_stats, y32_stats)
        assert ok
        # the repacked images: a second policy object created from the read-back arrays computes the same bits on the all-zero observation
        # (biases and padding only), on ordinary rows, and on rows with large entries, which a non-zero padding weight or bias would show up in
        fresh = GaussianActorCritic(got[:12], got[12], activation=activation, lo=-1.0, seed=5).attach(eng)
        x = np.concatenate([np.zeros((1, D), np.float32), case["obs"][:36], 50.0 * case["obs"][:40]])
        n = len(x)
        dx = _up(eng, x)
        out = [[eng.empty((n, P), np.float32), eng.empty((n,), np.float32)] for _ in range(2)]
        for ac, (m, v) in zip((dev.pol.ac, fresh.ac), out):
            eng.ac_forward(ac, dx, n, mean=m, value=v)
        eng.synchronize()
        for a, b in zip(*out):
            assert np.array_equal(_bits(a.to_host()), _bits(b.to_host()))
        # ... and after the sync it samples the same actions, clipped actions and log-probabilities from the same draws
        eng.ppo_sync(dev.learner)
        acts = [[eng.empty((n, P), np.float32), eng.empty((n, P), np.float32), eng.empty((n,), np.float32)] for _ in range(2)]
        for ac, (a, c, lp) in zip((dev.pol.ac, fresh.ac), acts):
            eng.ac_seed(ac, 11, 3)
            eng.ac_act(ac, dx, n, actions=a, clipped=c, log_prob=lp)
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


# ---- the rate setters ----
@pytest.fixture(scope="module")
def pst_case(eng):
    case = make_case(eng.D, eng.P, n_rows=N_ROWS["tanh"])
    assert (eng.D, eng.P) == learner_cases.SHAPES["pst"]
    return case


@pytest.mark.parametrize("new_clip", [0.6, 0.03])
def test_set_rates_changes_the_clip_range_of_the_next_gradient(eng, pst_case, new_clip):
    """A gradient at the create-time clip 0.2, ev2g_ppo_set_rates, the gradient again; no apply in between, so the ratios do not move.  On the
    float64 reference alone, first: no ratio within 0.01 of a boundary of the new clip, and the two references at least 1000 tolerances apart
    on pi_W1, action_W and log_std, so a setter that did nothing (or waited for the next create) cannot pass."""
    import torch
    case = pst_case
    idx = _index_sets(_grid_cap(case), N_ROWS["tanh"])[4]
    assert len(idx) == 97
    cfg = dict(vf_coef=0.5, ent_coef=0.0, normalize_advantage=True)
    refs = {c: reference(case, idx, clip=c, **cfg) for c in (CLIP, new_clip)}
    y32s = {c: torch_grads(case, idx, torch.float32, clip=c, **cfg) for c in (CLIP, new_clip)}
    check_branches(refs[CLIP][2])
    ratio = refs[new_clip][2]["ratio"]
    gap = float(np.minimum(np.abs(ratio - (1.0 - new_clip)), np.abs(ratio - (1.0 + new_clip))).min())
    _record(f"RATES clip {CLIP} -> {new_clip}: smallest distance of a ratio from a boundary {gap:.4f}; clip_fraction {refs[CLIP][1][5]:.3f} -> "
            f"{refs[new_clip][1][5]:.3f}")
    assert gap > 0.01 and refs[CLIP][1][5] != refs[new_clip][1][5]
    for name in ("pi_W1", "action_W", "log_std"):
        k = NAMES.index(name)
        r_old, r_new = refs[CLIP][0][k], refs[new_clip][0][k]
        diff = float(np.abs(r_new - r_old).max())
        tol = max(grad_tol(refs[c][0][k], float(np.abs(y32s[c][0][k] - refs[c][0][k]).max())) for c in (CLIP, new_clip))
        _record(f"RATES clip {CLIP} -> {new_clip} {name}: the references differ by {diff:.3e}, tol {tol:.3e}")
        assert diff >= 1000.0 * tol, name
    dev = learner_cases._Device("ppo", eng, case, **cfg)   # (created at clip_range=CLIP)
    try:
        ok = True
        for c in (CLIP, new_clip):
            if c != CLIP:
                eng.ppo_set_rates(dev.ppo, 3e-4, c)
            got, got_stats = dev.grad(idx)
            ok &= _compare_grads(f"RATES clip {c}", got, got_stats, refs[c][0], refs[c][1], *y32s[c])
        assert ok
    finally:
        dev.close()


PPO_LRS = (3e-4, 1e-3, 1e-4)
A2C_LRS = (7e-4, 2e-3, 1e-4)


def _minibatches():
    rng = np.random.default_rng(21)
    return [rng.choice(N_ROWS["tanh"], B, replace=False) for B in (64, 95, 33)]


def _lr_is_seen(tag, ref, y32, train, lrs, **loop):
    """On the float64 loop alone: with the create-time rate kept (lrs[0] at every step) some array ends at least a hundred of its tolerances
    from where the per-step rates take it (the rates differ by factors of 3 and more, so the distance is of the order of the steps themselves:
    no rounding closes it), so a setter without effect cannot pass."""
    import torch
    kept, _, _ = train(torch.float64, lrs=[lrs[0]] * len(lrs), **loop)
    far = max(float(np.abs(k - r).max()) / float(value_tol(r, float(np.abs(y - r).max())).max()) for k, r, y in zip(kept, ref, y32))
    _record(f"RATES {tag}: the float64 loop at the create-time rate ends {far:.1f} tolerances from the scheduled one")
    assert far >= 100.0


def test_set_rates_changes_the_learning_rate_of_the_next_step(eng, pst_case):
    import torch
    case, sets = pst_case, _minibatches()
    cfg = dict(vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
    train = lambda dtype, lrs, **kw: torch_train(case, sets, dtype, lr=lrs[0], lrs=lrs, **kw)  # noqa: E731
    ref, ref_stats, _ = train(torch.float64, PPO_LRS, **cfg)
    y32, y32_stats, _ = train(torch.float32, PPO_LRS, **cfg)
    _lr_is_seen("ppo", ref, y32, train, PPO_LRS, **cfg)
    dev = learner_cases._Device("ppo", eng, case, lr=PPO_LRS[0], **cfg)
    try:
        stats = []
        for lr, ix in zip(PPO_LRS, sets):
            eng.ppo_set_rates(dev.ppo, lr, CLIP)
            stats.append(dev.step(ix))
        ok = _compare_params(f"RATES ppo lr {PPO_LRS}", dev.weights(), ref, y32, _start(case))
        ok &= _compare_step_stats(f"RATES ppo lr {PPO_LRS}", np.array(stats), ref_stats, y32_stats)
        assert ok
    finally:
        dev.close()


@pytest.mark.parametrize("use_rms_prop", [True, False], ids=["rmsprop", "adam"])
def test_a2c_set_rate_changes_the_learning_rate_of_the_next_update(eng, pst_case, use_rms_prop):
    import torch
    case, sets = pst_case, _minibatches()
    cfg = dict(vf_coef=0.5, ent_coef=0.01, normalize_advantage=True, use_rms_prop=use_rms_prop)
    train = lambda dtype, lrs, **kw: a2c_torch_train([case] * 3, sets, dtype, lr=lrs[0], lrs=lrs, **kw)  # noqa: E731
    ref, ref_stats, _ = train(torch.float64, A2C_LRS, **cfg)
    y32, y32_stats, _ = train(torch.float32, A2C_LRS, **cfg)
    tag = f"a2c {'RMSprop' if use_rms_prop else 'Adam'}"
    _lr_is_seen(tag, ref, y32, train, A2C_LRS, **cfg)
    dev = learner_cases._Device("a2c", eng, case, lr=A2C_LRS[0], **cfg)
    try:
        stats = []
        for lr, ix in zip(A2C_LRS, sets):
            eng.a2c_set_rate(dev.a2c, lr)
            stats.append(dev.step(ix))
        ok = _compare_params(f"RATES {tag} lr {A2C_LRS}", dev.weights(), ref, y32, _start(case))
        ok &= _compare_step_stats(f"RATES {tag} lr {A2C_LRS}", np.array(stats), ref_stats, y32_stats)
        assert ok
    finally:
        dev.close()


# ---- ... and through the Python learners behind a collector ----
def _collected_case(pol, batch, weights, log_std):
    f = lambda t, *s: t.reshape(-1, *s).cpu().numpy()  # noqa: E731
    return dict(weights=weights, log_std=log_std, activation=pol.activation, obs=f(batch.observations, pol.d_in), actions=f(batch.actions, pol.d_out),
                old_log_prob=f(batch.log_probs), advantages=f(batch.advantages), returns=f(batch.returns))


def _policy_behind_a_collector():
    from ev2gym_amd.onpolicy import GaussianActorCritic, init_ac_weights
    big = _gen_engine("pst", pool=3)
    w0, ls0 = init_ac_weights(big.D, big.P, seed=3), np.full(big.P, -0.5, np.float32)
    return big, GaussianActorCritic(w0, ls0, lo=0.0, seed=5).attach(big), list(w0) + [ls0]


def _state(learner):
    from ev2gym_amd.onpolicy import SB3_KEYS, SB3_LOG_STD
    sd = learner.state_dict()
    return [sd[k] for k in SB3_KEYS] + [sd[SB3_LOG_STD]]


def test_ppolearner_set_rates_reaches_the_device():
    """PPOLearner.set_rates before each of three train() calls of one minibatch each: the parameters read back through state_dict() against
    the float64 torch loop with the same rate per step."""
    import torch
    from ev2gym_amd.onpolicy import OnPolicyCollector
    from ev2gym_amd.ppo import PPOLearner
    big, pol, start = _policy_behind_a_collector()
    try:
        col = OnPolicyCollector(big, pol, 24)
        batch = col.collect().clone()
        rng = np.random.default_rng(2)
        sets = [rng.choice(24 * big.E, B, replace=False) for B in (64, 95, 33)]
        learner = PPOLearner(col, lr=PPO_LRS[0], n_epochs=1, batch_size=64)
        for lr, ix in zip(PPO_LRS, sets):
            learner.set_rates(lr=lr)
            learner.train(batch, minibatches=[ix])
        case = _collected_case(pol, batch, start[:12], start[12])
        train = lambda dtype, lrs, **kw: torch_train(case, sets, dtype, lr=lrs[0], lrs=lrs, **kw)  # noqa: E731
        ref, _, _ = train(torch.float64, PPO_LRS)
        y32, _, _ = train(torch.float32, PPO_LRS)
        _lr_is_seen("PPOLearner", ref, y32, train, PPO_LRS)
        assert (learner.lr, learner.clip_range) == (PPO_LRS[-1], CLIP)
        assert _compare_params(f"RATES PPOLearner lr {PPO_LRS}", _state(learner), ref, y32, start)
    finally:
        pol.close()
        big.close()


def test_a2clearner_set_rate_reaches_the_device():
    """A2CLearner.set_rate before each of three rollouts' train() (five steps each, one update over every row): as above."""
    import torch
    from ev2gym_amd.a2c import A2CLearner
    from ev2gym_amd.onpolicy import OnPolicyCollector
    big, pol, start = _policy_behind_a_collector()
    try:
        col = OnPolicyCollector(big, pol, n_steps=5, gae_lambda=1.0)
        learner = A2CLearner(col, lr=A2C_LRS[0])
        cases = []
        for lr in A2C_LRS:
            learner.set_rate(lr)
            batch = col.collect().clone()
            learner.train(batch)
            cases.append(_collected_case(pol, batch, start[:12], start[12]))
        rows = [np.arange(5 * big.E)] * 3
        train = lambda dtype, lrs, **kw: a2c_torch_train(cases, rows, dtype, lr=lrs[0], lrs=lrs, **kw)  # noqa: E731
        ref, _, _ = train(torch.float64, A2C_LRS)
        y32, _, _ = train(torch.float32, A2C_LRS)
        _lr_is_seen("A2CLearner", ref, y32, train, A2C_LRS)
        assert learner.lr == A2C_LRS[-1]
        assert _compare_params(f"RATES A2CLearner lr {A2C_LRS}", _state(learner), ref, y32, start)
    finally:
        pol.close()
        big.close()
