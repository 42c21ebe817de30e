"""Host side of the on-policy collector (csrc/ev2g_ac.h, ev2gym_amd/onpolicy.py): the GAE walk and the noise stream that host and device share
one source for, against their numpy restatements, and the SB3 state-dict mapping and shape refusals of GaussianActorCritic.  No GPU.

Stable-Baselines3 is not installed where these run: the key mapping is held to SB3's parameter NAMES (written out below), not to a live policy."""
import numpy as np
import pytest

E = 37


def _gae_case(k, seed):
    rng = np.random.default_rng(seed)
    reward = rng.normal(size=(k, E)) * 3.0
    values = rng.normal(size=(k, E)).astype(np.float32)
    starts = (rng.random((k, E)) < 0.2).astype(np.uint8)
    starts[0, ::3] = 1          # episodes that start at step 0 ...
    starts[k - 1, 1::4] = 1     # ... and at the last step
    last_values = rng.normal(size=E).astype(np.float32)
    last_dones = (rng.random(E) < 0.5).astype(np.uint8)
    assert 0 < last_dones.sum() < E
    return reward, values, starts, last_values, last_dones


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
@pytest.mark.parametrize("k", [1, 7])
def test_host_gae_equals_the_numpy_float32_restatement_bit_for_bit(k, gamma, lam):
    from ev2gym_amd.engine import host_gae
    from ev2gym_amd.onpolicy import gae_numpy
    case = _gae_case(k, 100 + k)
    adv, ret = host_gae(*case, gamma, lam)
    adv_np, ret_np = gae_numpy(*case, gamma, lam)
    assert adv.dtype == ret.dtype == np.float32 and adv.shape == (k, E)
    assert np.array_equal(adv.view(np.uint32), adv_np.view(np.uint32))
    assert np.array_equal(ret.view(np.uint32), ret_np.view(np.uint32))
    assert np.abs(adv).max() > 0.1   # (not a comparison of zeros)


def test_gae_restatement_is_sb3s_loop():
    """gae_numpy against SB3's compute_returns_and_advantage written out as SB3 has it (python floats gamma / gae_lambda, float32 arrays)."""
    from ev2gym_amd.onpolicy import gae_numpy
    reward, values, starts, last_values, last_dones = _gae_case(7, 5)
    gamma, gae_lambda = 0.99, 0.95
    rewards, episode_starts = reward.astype(np.float32), starts.astype(np.float32)
    advantages = np.zeros_like(values)
    last_gae_lam = 0
    for step in reversed(range(7)):
        if step == 6:
            next_non_terminal = 1.0 - last_dones.astype(np.float32)
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    adv, ret = gae_numpy(reward, values, starts, last_values, last_dones, gamma, gae_lambda)
    assert np.array_equal(adv, advantages) and np.array_equal(ret, advantages + values)


def test_host_normal_is_a_counter_based_stream():
    from ev2gym_amd.engine import host_normal
    a = host_normal(1000, 42)
    assert a.dtype == np.float32
    assert np.array_equal(a.view(np.uint32), host_normal(1000, 42).view(np.uint32))
    assert not np.array_equal(a, host_normal(1000, 43))
    # first_index is an offset into the same stream: two halves are the whole
    assert np.array_equal(np.concatenate([host_normal(400, 42, 0), host_normal(600, 42, 400)]).view(np.uint32), a.view(np.uint32))


def test_host_normal_is_box_muller_on_host_uniforms_draws():
    from ev2gym_amd.engine import host_normal, host_uniform
    n, first = 20000, 123
    u = host_uniform(2 * (first + n), 9, 0.0, 1.0)[2 * first:]
    ref = np.sqrt(-2.0 * np.log(1.0 - u[0::2])) * np.cos(2.0 * np.pi * u[1::2])
    got = host_normal(n, 9, first).astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(got - ref) / ulp))
    print(f"host_normal vs float64 Box-Muller: {worst:.3f} ulp")
    assert worst <= 4.0


def test_host_normal_moments():
    from ev2gym_amd.engine import host_normal
    N = 1 << 20
    z = host_normal(N, 7).astype(np.float64)
    mean, var = z.mean(), z.var()
    print(f"N = 2^20: mean {mean:.3e} (bound {5 / np.sqrt(N):.3e}), var - 1 {var - 1:.3e} (bound {5 * np.sqrt(2 / N):.3e})")
    # five-sigma bounds of the two estimators
    assert abs(mean) < 5.0 / np.sqrt(N)
    assert abs(var - 1.0) < 5.0 * np.sqrt(2.0 / N)


# ---- GaussianActorCritic: the numpy path needs no device ----
SB3_NAMES = {   # ActorCriticPolicy(net_arch=dict(pi=[h1, h2], vf=[v1, v2])).state_dict() -> (position in ev2g_ac_create's order, shape)
    "mlp_extractor.policy_net.0.weight": (0, "h1,D"), "mlp_extractor.policy_net.0.bias": (1, "h1"),
    "mlp_extractor.policy_net.2.weight": (2, "h2,h1"), "mlp_extractor.policy_net.2.bias": (3, "h2"),
    "mlp_extractor.value_net.0.weight": (4, "v1,D"), "mlp_extractor.value_net.0.bias": (5, "v1"),
    "mlp_extractor.value_net.2.weight": (6, "v2,v1"), "mlp_extractor.value_net.2.bias": (7, "v2"),
    "action_net.weight": (8, "P,h2"), "action_net.bias": (9, "P"), "value_net.weight": (10, "one,v2"), "value_net.bias": (11, "one"),
}


def _state_dict(D=11, h1=6, h2=7, v1=8, v2=9, P=3, seed=0):
    rng = np.random.default_rng(seed)
    dims = dict(D=D, h1=h1, h2=h2, v1=v1, v2=v2, P=P, one=1)
    sd = {k: rng.normal(size=tuple(dims[s] for s in shape.split(","))).astype(np.float32) for k, (_, shape) in SB3_NAMES.items()}
    sd["log_std"] = rng.uniform(-1, 0, P).astype(np.float32)
    return sd


def test_state_dict_keys_map_to_the_create_order():
    from ev2gym_amd.onpolicy import SB3_KEYS, GaussianActorCritic, ac_forward_numpy
    sd = _state_dict()
    assert set(SB3_KEYS) == set(SB3_NAMES) and all(SB3_KEYS[i] == k for k, (i, _) in SB3_NAMES.items())
    shuffled = {k: sd[k] for k in reversed(list(sd))}   # (the order of the dict does not matter, the names do)
    pol = GaussianActorCritic.from_state_dict(shuffled, activation="tanh", lo=-1.0)
    assert (pol.d_in, pol.h1, pol.h2, pol.v1, pol.v2, pol.d_out) == (11, 6, 7, 8, 9, 3)
    for k, (i, _) in SB3_NAMES.items():
        assert np.array_equal(pol.weights[i], sd[k]), k
    assert np.array_equal(pol.log_std, sd["log_std"])
    assert set(pol.state_dict()) == set(sd)
    # torch tensors are accepted like arrays
    import torch
    pol_t = GaussianActorCritic.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    assert all(np.array_equal(a, b) for a, b in zip(pol.weights, pol_t.weights))
    # the float64 forward is the two trunks with their own heads
    x = np.random.default_rng(1).normal(size=(5, 11))
    mean, value = pol.forward_numpy(x)
    w = [sd[k].astype(np.float64) for k in SB3_KEYS]
    hp = np.tanh(np.tanh(x @ w[0].T + w[1]) @ w[2].T + w[3])
    hv = np.tanh(np.tanh(x @ w[4].T + w[5]) @ w[6].T + w[7])
    assert mean.shape == (5, 3) and value.shape == (5,)
    assert np.allclose(mean, hp @ w[8].T + w[9], rtol=0, atol=1e-14) and np.allclose(value, (hv @ w[10].T + w[11])[:, 0], rtol=0, atol=1e-14)
    relu = ac_forward_numpy(x, pol.weights, "relu")[0]
    assert not np.allclose(relu, mean)


def test_state_dict_refusals():
    from ev2gym_amd.onpolicy import GaussianActorCritic
    sd = _state_dict()
    short = {k: v for k, v in sd.items() if k != "value_net.bias"}
    with pytest.raises(KeyError, match="value_net.bias"):
        GaussianActorCritic.from_state_dict(short)
    with pytest.raises(KeyError, match="log_std"):
        GaussianActorCritic.from_state_dict({k: v for k, v in sd.items() if k != "log_std"})
    deep = dict(sd)
    deep["mlp_extractor.policy_net.4.weight"] = np.zeros((4, 7), np.float32)
    with pytest.raises(ValueError, match="more than two hidden layers"):
        GaussianActorCritic.from_state_dict(deep)


@pytest.mark.parametrize("kw,field", [(dict(D=193), "d_in"), (dict(h1=257), "h1"), (dict(h2=257), "h2"), (dict(v1=257), "v1"), (dict(v2=257), "v2"),
                                      (dict(P=65), "d_out")])
def test_shapes_outside_the_kernels_range_are_refused(kw, field):
    from ev2gym_amd.onpolicy import GaussianActorCritic
    with pytest.raises(ValueError, match=field + r" \d+ is outside"):
        GaussianActorCritic.from_state_dict(_state_dict(**kw))
    edge = {k: {"D": 192, "P": 64}.get(k, 256) for k in kw}   # the limit itself is accepted
    GaussianActorCritic.from_state_dict(_state_dict(**edge))


def test_inconsistent_arrays_and_settings_are_refused():
    from ev2gym_amd.onpolicy import GaussianActorCritic
    sd = _state_dict()
    bad = dict(sd)
    bad["mlp_extractor.value_net.2.weight"] = np.zeros((9, 5), np.float32)
    with pytest.raises(ValueError, match=r"vf_W2 has shape \(9, 5\), expected \(9, 8\)"):
        GaussianActorCritic.from_state_dict(bad)
    bad = dict(sd)
    bad["action_net.bias"] = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="action_b"):
        GaussianActorCritic.from_state_dict(bad)
    bad = dict(sd)
    bad["log_std"] = np.array([0.0, np.nan, 0.0], np.float32)
    with pytest.raises(ValueError, match="log_std is not finite"):
        GaussianActorCritic.from_state_dict(bad)
    bad["log_std"] = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="log_std has shape"):
        GaussianActorCritic.from_state_dict(bad)
    with pytest.raises(ValueError, match="activation"):
        GaussianActorCritic.from_state_dict(sd, activation="gelu")
    with pytest.raises(ValueError, match="lo 0.5"):
        GaussianActorCritic.from_state_dict(sd, lo=0.5)
    pol = GaussianActorCritic.from_state_dict(sd)
    with pytest.raises(ValueError, match="log_std is not finite"):
        pol.set_log_std([0.0, np.inf, 0.0])
    with pytest.raises(ValueError, match="shapes differ"):
        pol.set_weights(GaussianActorCritic.from_state_dict(_state_dict(h1=5)).weights)
