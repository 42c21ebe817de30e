"""The actor-critic's thirteen parameter arrays through every host path that places them (ev2g_ac_create, ev2g_ac_set_weights,
ev2g_ac_set_log_std, ev2g_ac_get_weights, ev2g_ppo_create, ev2g_ppo_get_grads): the packed images read back, and a bound learner's masters and
transposed images after the policy's weights are replaced.

The network is the smallest in which every dimension has padding and the two trunks differ: d_in 9, h (33, 17), v (40, 7), d_out 3.  None of
the calls steps the env, so any loaded engine serves.  Every comparison is bit for bit: the images hold the float32 values themselves, and the
learner's kernels have one fixed summation order and no float atomics (the same call on the same state gives the same bits), so a policy whose
weights were replaced and a fresh policy created from the replacement are the same state as long as Adam has not stepped (t = 0, m = v = 0)."""
import numpy as np
import pytest

from tests.test_onpolicy_gpu import _bits, _gen_engine, _up

pytestmark = pytest.mark.gpu

SHAPE = (9, 33, 17, 40, 7, 3)   # d_in, h1, h2, v1, v2, d_out
NAMES = ("pi_W1", "pi_b1", "pi_W2", "pi_b2", "vf_W1", "vf_b1", "vf_W2", "vf_b2", "action_W", "action_b", "value_W", "value_b", "log_std")
N_ROWS = 37


@pytest.fixture(scope="module")
def eng():
    e = _gen_engine("pst")
    yield e
    e.close()


def _arrays(seed):
    """(twelve arrays, log_std) of SHAPE, every element a normal float32 that is not zero"""
    from ev2gym_amd.onpolicy import init_ac_weights
    D, h1, h2, v1, v2, P = SHAPE
    w = init_ac_weights(D, P, seed=seed, h=(h1, h2), v=(v1, v2))
    for a in w:
        a[a == 0] = np.float32(0.125)
    ls = np.random.default_rng(seed + 100).uniform(-1.0, 0.0, P).astype(np.float32)
    return w, ls


def _same(tag, got, want):
    assert len(got) == len(want) == 13
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == np.float32, f"{tag}: {name} {g.shape} {g.dtype}"
        bad = int((_bits(g) != _bits(w)).sum())
        assert bad == 0, f"{tag}: {name} differs in {bad} of {g.size} elements"


def _read(eng, ac):
    w, ls = eng.ac_get_weights(ac, SHAPE)
    return w + [ls]


def test_a_policy_without_a_learner_returns_the_created_arrays(eng):
    for activation in ("tanh", "relu"):
        w, ls = _arrays(1)
        ac = eng.ac_create(w, ls, activation=activation)
        try:
            _same(f"created ({activation})", _read(eng, ac), w + [ls])
            w2, ls2 = _arrays(2)
            eng.ac_set_weights(ac, w2)
            eng.ac_set_log_std(ac, ls2)
            _same(f"replaced ({activation})", _read(eng, ac), w2 + [ls2])
        finally:
            eng.ac_destroy(ac)


def _rows():
    rng = np.random.default_rng(7)
    D, P = SHAPE[0], SHAPE[5]
    obs = rng.uniform(0.0, 1.0, (N_ROWS, D)).astype(np.float32)
    actions = rng.uniform(-1.0, 1.0, (N_ROWS, P)).astype(np.float32)
    old_lp = rng.uniform(-4.0, -2.0, N_ROWS).astype(np.float32)
    adv = rng.normal(0.0, 1.0, N_ROWS).astype(np.float32)
    ret = rng.normal(0.0, 1.0, N_ROWS).astype(np.float32)
    idx = rng.permutation(N_ROWS).astype(np.int32)
    idx[5] = idx[0]   # one duplicate
    return obs, actions, old_lp, adv, ret, idx


def _forward(eng, ac, x):
    n, P = x.shape[0], SHAPE[5]
    dx, dm, dv = _up(eng, x), eng.empty((n, P), np.float32), eng.empty((n,), np.float32)
    eng.ac_forward(ac, dx, n, mean=dm, value=dv)
    eng.synchronize()
    out = dm.to_host(), dv.to_host()
    for b in (dx, dm, dv):
        b.free()
    return out


@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_replaced_weights_reach_a_bound_learner_like_a_fresh_one(eng, activation):
    w1, ls1 = _arrays(1)
    w2, ls2 = _arrays(2)
    cfg = dict(lr=1e-2, ent_coef=0.01)
    moved = eng.ac_create(w1, ls1, activation=activation)
    fresh = eng.ac_create(w2, ls2, activation=activation)
    bufs = [_up(eng, a) for a in _rows()]
    try:
        ppo_moved = eng.ppo_create(moved, **cfg)
        _same("the masters at create", _read(eng, moved), w1 + [ls1])
        eng.ac_set_weights(moved, w2)
        eng.ac_set_log_std(moved, ls2)
        _same("the masters after set_weights / set_log_std", _read(eng, moved), w2 + [ls2])
        ppo_fresh = eng.ppo_create(fresh, **cfg)
        grads = []
        for ppo in (ppo_moved, ppo_fresh):
            eng.ppo_grad(ppo, *bufs, N_ROWS)
            grads.append(eng.ppo_get_grads(ppo, SHAPE))
        assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in grads[1])
        _same("the gradient", grads[0], grads[1])   # (a stale transposed image changes the first layers' gradients)
        for ppo in (ppo_moved, ppo_fresh):
            eng.ppo_apply(ppo)
        after = _read(eng, fresh)
        assert all((_bits(a) != _bits(b)).any() for a, b in zip(after, w2 + [ls2])), "the step moved every array"
        _same("the masters after one step", _read(eng, moved), after)
        x = np.random.default_rng(8).uniform(0.0, 1.0, (5, SHAPE[0])).astype(np.float32)
        x[0] = 0.0
        (m0, v0), (m1, v1) = _forward(eng, moved, x), _forward(eng, fresh, x)
        assert np.isfinite(m1).all() and np.isfinite(v1).all()
        assert (_bits(m0) == _bits(m1)).all() and (_bits(v0) == _bits(v1)).all(), "the forward from the rewritten images"
    finally:
        for b in bufs:
            b.free()
        eng.ac_destroy(moved)   # (a bound learner goes with its policy)
        eng.ac_destroy(fresh)
