"""Every entry of the step kernels' launch tables (csrc/ev2g_host.hip: kWaveTable, v2_kernel, kFusedTable, indexed by csrc/ev2g_route_host.h)
computes what its name says.  A wrong entry is silent -- a kernel with another compiled-in state, reward or action format launched under the
right specialisation number -- so every plugin pair runs through every instantiation a launch can reach, against the C oracle
(oracle/ev2g_oracle.c) or, for the fused actor + step launch, against the two-launch chain.

Pools are tiny: 6-step episodes cut from generated ones, with EVs arriving in steps 0 and 1 and leaving from step 3 on, so that a 3-step run
charges, discharges and scores them.  Actions are float32 values, the same for the float64 and the float32 hand-over instantiations."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOADS, PST, PMAX = "V2G_profit_max_loads", "PublicPST", "V2G_profit_max"
STATES = [LOADS, PST, PMAX]
COMPILED = ["ProfitMax_TrPenalty_UserIncentives", "SquaredTrackingErrorReward", "profit_maximization"]   # reward kinds 0, 1, 2
RUN_TIME = "SquaredTrackingErrorRewardWithPenalty"                                                       # kind 4: the shared run-time instantiation
T, SEED, W0 = 6, 3, 6   # episode length; the generator seed (chosen on the CPU with the oracle: _rewards_differ holds for all three states); the window's first step
F32_ULP = 2.0 ** -23    # a float32 row is the rounded float64 one: two float64 values within 1e-9 of each other may round to neighbouring float32 values


def make_pool(state, E, C, R=1, seed=SEED):
    """A T-step pool: steps [W0, W0 + T) of a generated 40-step batch that starts at 08:00; of every env, the first session of each charger,
    re-timed to arrive in step 0 or 1 (time_of_arrival 1 or 2) and to leave at step 3 or 4 (inside what the generator itself draws: it keeps
    departures below T - 1)."""
    from ev2gym_amd import _abi
    from ev2gym_amd.scenario import ScenarioBatch
    from ev2gym_amd.scenario_gen import GenConfig, generate
    kw = dict(simulation_length=40, hour=8, spawn_multiplier=30.0 if state == PST else 10.0, seed=seed)
    long = generate(GenConfig.public_pst(E, C, **kw) if state == PST else GenConfig.v2g_profit_plus_loads(E, C, R, demand_response=False, **kw))
    a, new = long.finalize().arrays, {}
    st = a["env_session_start"]
    keep, t_arr, t_dep, start = [], [], [], [0]
    for e in range(E):
        ids = np.arange(st[e], st[e + 1])
        first = ids[np.unique(a["ev_cs"][ids], return_index=True)[1]]   # by charger
        first = np.sort(first)                                          # back in arrival order
        late = np.arange(len(first)) >= (len(first) + 1) // 2           # the later half arrives one step later
        order = np.lexsort((a["ev_cs"][first], late))
        keep.append(first[order]); t_arr.append(1 + late[order].astype(int)); t_dep.append(2 + (np.arange(len(first)) % 3))
        start.append(start[-1] + len(first))
    keep = np.concatenate(keep)
    for name, _ in _abi.BATCH_ARRAYS:
        v = a[name]
        if name.startswith("ev_"):
            new[name] = v[keep].copy()
        elif name in ("charge_price", "discharge_price", "power_setpoints") or (name.startswith("tr_") and v.ndim == 3 and v.shape[-1] == long.n_steps):
            new[name] = v[..., W0:W0 + T].copy()
        else:
            new[name] = v.copy()
    new["ev_t_arr"], new["ev_t_dep"] = np.concatenate(t_arr).astype(np.int32), np.concatenate(t_dep).astype(np.int32)
    new["env_session_start"] = np.asarray(start, np.int64)
    new["tr_n_dr"] = np.zeros_like(a["tr_n_dr"])
    new["tr_max_power"] *= 0.1   # tight transformers: some steps overload them, the one term that tells ProfitMax_TrPenalty_UserIncentives from profit_maximization
    pool = ScenarioBatch(E, T, long.timescale, long.n_chargers, long.ports_per_charger, long.n_transformers, long.v2g_enabled, long.horizon, new)
    print("sessions", np.diff(start)); assert min(np.diff(start)) >= C // 4, "too few sessions in the generated batch"
    return pool.finalize()


def actions_for(state, k, E, P, seed=11):
    from ev2gym_amd.engine import host_uniform
    return host_uniform(k * E * P, seed, 0.0 if state == PST else -1.0, 1.0).reshape(k, E, P).astype(np.float32)


def oracle_run(pool, rk, sk, acts, k):
    """k oracle steps: the rows of every step, the state of every env, the 17 statistics."""
    from oracle.oracle import Oracle
    ora = Oracle(pool, rk, sk)
    out = dict(obs0=ora.reset(), obs=[], reward=[], done=[], mask=[])
    for t in range(k):
        o, r, d, m, rc = ora.step(acts[t].astype(np.float64))
        assert rc == 0
        for key, v in zip(("obs", "reward", "done", "mask"), (o, r, d, m)):
            out[key].append(v)
    for key in ("obs", "reward", "done", "mask"):
        out[key] = np.stack(out[key])
    out["peek"] = [ora.peek(e) for e in range(pool.n_envs)]
    out["stats"] = ora.stats()
    ora.close()
    return out


def _close(a, b, what, tol=1e-9):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all(), f"{what}: NaN pattern differs"
    err = np.nan_to_num(np.abs(a - b) / np.maximum(1.0, np.abs(np.nan_to_num(b))))
    print(f"    {what}: max rel err {err.max(initial=0.0):.3e}")
    assert err.max(initial=0.0) <= tol, f"{what}: max rel err {err.max():.3e}"


# (the charger-level accumulators exist only with EV2G_FLAG_LOG_CS_HISTORY, which rules the full instantiations out)
_PEEK = [("port_capacity", "cap"), ("port_energy", "energy"), ("port_current", "current"), ("port_total_energy", "tot_e"), ("port_prev_power", "prev_power"),
         ("tr_power", "tr_power"), ("tr_overload", "tr_overload"), ("power_usage", "usage"), ("power_potential", "potential")]


def check_state(eng, ref, tag, k):
    """Port state, charger accumulators and the histories of every env, and the statistics of the running episode, after k steps."""
    for e in range(eng.E):
        pk, po = eng.peek(e), ref["peek"][e]
        assert pk["current_step"] == k
        assert (pk["port_cycles"] == po["cycles"]).all() and (pk["port_session"] == po["session"]).all(), f"{tag}: env {e} sessions"
        err = max(np.nan_to_num(np.abs(pk[a] - po[b]) / np.maximum(1.0, np.abs(po[b]))).max(initial=0.0) for a, b in _PEEK)
        assert err <= 1e-9, (tag, e, {a: float(np.abs(pk[a] - po[b]).max(initial=0.0)) for a, b in _PEEK})
    _close(eng.stats(), ref["stats"], f"{tag}: statistics")
    eng.check_faults()


_POOLS, _REFS = {}, {}


def pool_and_reference(state, reward, E, C, k):
    """One pool per (state, shape) and one oracle run per (pool, reward), shared by the cases."""
    from ev2gym_amd import _abi
    if (state, E, C) not in _POOLS:
        _POOLS[state, E, C] = make_pool(state, E, C)
    pool = _POOLS[state, E, C]
    acts = actions_for(state, k, E, pool.n_ports)
    if (state, reward, E, C, k) not in _REFS:
        _REFS[state, reward, E, C, k] = oracle_run(pool, _abi.REWARD_KINDS[reward], _abi.STATE_KINDS[state], acts, k)
    return pool, acts, _REFS[state, reward, E, C, k]


# ---- ev2g_step_wave: (state, reward slot, action format, full / wide / strided) ----
E_WAVE, P_WAVE, K_WAVE = 5, 32, 3   # a partial workgroup (two envs per wavefront, eight per workgroup); the smallest width that is wide for all three states


def test_the_three_compiled_in_rewards_differ_on_the_pool():
    """What makes a swapped reward visible below: on the oracle's own output the three compiled-in rewards differ pairwise, in every state's pool, at
    some step of the run."""
    for state in STATES:
        r = [pool_and_reference(state, rw, E_WAVE, P_WAVE, K_WAVE)[2]["reward"] for rw in COMPILED]
        for i in range(3):
            for j in range(i + 1, 3):
                gap = np.abs(r[i] - r[j]).max(axis=1)
                print(f"{state}: |{COMPILED[i]} - {COMPILED[j]}| per step {gap}")
                assert (np.abs(r[i] - r[j]) > 1e-6 * np.maximum(1.0, np.abs(r[j]))).any(), (state, COMPILED[i], COMPILED[j])
        mask = pool_and_reference(state, COMPILED[0], E_WAVE, P_WAVE, K_WAVE)[2]["mask"]
        assert mask[0].any(axis=1).all() and mask.sum() > mask[0].sum(), "every env holds EVs from step 0 on, and more arrive"


# (switch at load time, float32 hand-over, strided outputs) -> the specialisation a compiled-in reward gets; a run-time reward gets 0 everywhere
VARIANTS = [("EV2G_NO_FULL", False, True, 0), ("EV2G_NO_FULL", True, False, 0), ("EV2G_NO_WIDE", False, False, 1), ("EV2G_NO_WIDE", True, False, 1),
            (None, False, False, 2), (None, True, False, 2), (None, False, True, 3)]


@pytest.mark.parametrize("reward", COMPILED + [RUN_TIME])
@pytest.mark.parametrize("state", STATES)
def test_every_wave_instantiation_against_the_oracle(state, reward, monkeypatch):
    """One persistent launch of 3 steps through each instantiation the pair has -- general float64 (strided outputs: every row kept), general with
    the float32 hand-over, full and full + wide in both formats, wide with strided float64 outputs -- on 5 envs of 32 ports.  Rows against the
    oracle: float64 to 1e-9, masks and done flags exact, the float32 observation to one float32 ulp; stride-0 launches leave their last step's
    rows, so every launch is also held to the oracle's port state, charger accumulators, histories and statistics (the episode return among them:
    the sum of all three rewards) after the third step."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    E, k = E_WAVE, K_WAVE
    pool, acts, ref = pool_and_reference(state, reward, E, P_WAVE, k)
    rk, sk = _abi.REWARD_KINDS[reward], _abi.STATE_KINDS[state]
    for switch in (None, "EV2G_NO_WIDE", "EV2G_NO_FULL"):
        for s in ("EV2G_NO_FULL", "EV2G_NO_WIDE"):
            monkeypatch.delenv(s, raising=False)
        if switch:
            monkeypatch.setenv(switch, "1")
        eng = Engine(pool, rk, sk, device=0, flags=_abi.FLAG_LOG_SOC)
        monkeypatch.delenv(switch, raising=False) if switch else None
        assert eng.kernel_name == f"ev2g_step_wave<{sk},{min(rk, 3)}>" and (eng.E, eng.P, eng.T) == (E, P_WAVE, T)
        P, D = eng.P, eng.D
        a64, a32 = eng.empty((k, E, P)).upload(acts.astype(np.float64)), eng.empty((k, E, P), np.float32).upload(acts)
        o64, o32 = eng.empty((k, E, D)), eng.empty((E, D), np.float32)
        rew, done, mask = eng.empty((k, E)), eng.empty((k, E), np.uint8), eng.empty((k, E, P), np.uint8)
        for sw, f32, strided, want in VARIANTS:
            if sw != switch:
                continue
            want = want if rk < 3 else 0
            tag = f"{state} / {reward} / {sw or 'default'}{' float32' if f32 else ''}{' strided' if strided else ''}"
            print(tag)
            for b in (o64, rew):
                b.upload(np.full(b.shape, np.nan))
            o32.upload(np.full(o32.shape, np.nan, np.float32))
            eng.set_extras(obs_f32=o32, actions_f32=a32) if f32 else eng.set_extras()
            eng.reset()
            s = (E * D, E, E, E * P) if strided else (0, 0, 0, 0)
            eng.step_n(k, None if f32 else a64, E * P, None if f32 else o64, s[0], rew, s[1], done, s[2], mask, s[3], auto_reset=False, persistent=True)
            assert eng.last_launch_specialisation == want, (tag, eng.last_launch_specialisation)
            rows = range(k) if strided else [k - 1]
            got_r, got_d, got_m = rew.to_host(), done.to_host(), mask.to_host()
            for i, t in enumerate(rows):
                _close(got_r[i], ref["reward"][t], f"{tag}: reward[{t}]")
                assert np.array_equal(got_d[i], ref["done"][t]) and np.array_equal(got_m[i], ref["mask"][t]), f"{tag}: done / mask [{t}]"
                if f32:
                    _close(o32.to_host(), ref["obs"][t].astype(np.float32), f"{tag}: float32 obs[{t}]", tol=F32_ULP)
                else:
                    _close(o64.to_host()[i], ref["obs"][t], f"{tag}: obs[{t}]")
            check_state(eng, ref, tag, k)
        eng.close()


# ---- the fused actor + step launch: (state, reward, envs per wavefront, policy precision) ----
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("reward", COMPILED)
@pytest.mark.parametrize("state", STATES)
def test_every_fused_instantiation_equals_the_two_launch_chain(state, reward, precision, monkeypatch):
    """ev2g_rollout of 3 steps on 5 envs as ONE launch and, with EV2G_NO_FUSED=1 set for the call, as the chain of two launches per step: rewards,
    done flags, masks and the float32 observation and action rows bit for bit (the bar of tests/test_round6_gpu.py), specialisation 4 on the fused
    side only.  PublicPST at 20 ports, the widest its 64-input packing takes: under the bf16 policy that is the instantiation with two envs per
    wavefront (the one-env bf16 PublicPST entries exist but no network ev2g_mlp_create packs for this state reaches them: wider envs need the
    192-input packing); the head-table states at 32 ports (an even row width)."""
    from ev2gym_amd import _abi
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import Engine
    E, k, C = 5, 3, 20 if state == PST else 32
    if (state, E, C) not in _POOLS:
        _POOLS[state, E, C] = make_pool(state, E, C)
    pool = _POOLS[state, E, C]
    monkeypatch.delenv("EV2G_NO_FUSED", raising=False)
    monkeypatch.delenv("EV2G_NO_FUSED_F32", raising=False)
    eng = Engine(pool, _abi.REWARD_KINDS[reward], _abi.STATE_KINDS[state], device=0, flags=_abi.FLAG_LOG_SOC)
    P, D = eng.P, eng.D
    assert D % 2 == 0 or state == PST
    mlp = eng.mlp_create(*init_mlp_weights(D, P, seed=9), out_lo=0.0 if state == PST else -1.0, precision=precision)
    o32, a32 = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
    rew, done, mask = eng.empty((k, E)), eng.empty((k, E), np.uint8), eng.empty((k, E, P), np.uint8)
    eng.set_extras(obs_f32=o32, actions_f32=a32)
    runs = {}
    for fused in (True, False):
        if not fused:
            monkeypatch.setenv("EV2G_NO_FUSED", "1")
        rew.upload(np.full(rew.shape, np.nan)); a32.upload(np.full(a32.shape, np.nan, np.float32))
        eng.reset_f32(o32, 0)
        eng.rollout(mlp, k, rew, E, done, E, mask, E * P)
        assert (eng.last_launch_specialisation == 4) == fused, (fused, eng.last_launch_specialisation)
        eng.check_faults()
        runs[fused] = dict(reward=rew.to_host(), done=done.to_host(), mask=mask.to_host(), obs32=o32.to_host(), act32=a32.to_host(), stats=eng.stats().copy())
        monkeypatch.delenv("EV2G_NO_FUSED", raising=False)
    eng.mlp_destroy(mlp)
    eng.close()
    one, two = runs[True], runs[False]
    assert np.isfinite(two["reward"]).all() and np.isfinite(two["obs32"]).all() and np.abs(two["act32"]).max() > 0.01 and two["mask"].any()
    for key in two:
        assert np.array_equal(one[key], two[key], equal_nan=True), f"{state} / {reward} / {precision}: {key} differs between the fused launch and the chain"


# ---- the general kernels: ev2g_step_v2<256 / 512 / 1024, SPEC> and ev2g_step_big ----
@pytest.mark.parametrize("C,no_big,name,spec", [(65, False, "ev2g_step_v2<256>", 1), (257, False, "ev2g_step_v2<512>", 1), (513, True, "ev2g_step_v2<1024>", 1),
                                                (513, False, "ev2g_step_v2<1024>", 5)])
def test_every_general_kernel_entry_against_the_oracle(C, no_big, name, spec, monkeypatch):
    """The smallest env each block takes, 3 envs, 2 steps of the default plugin pair: a stride-0 launch gets the specialised instantiation (5:
    ev2g_step_big, unless EV2G_NO_BIG is set at load time), a launch with strided outputs the plain one, on the same load."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    E, k = 3, 2
    pool, acts, ref = pool_and_reference(LOADS, COMPILED[0], E, C, k)
    monkeypatch.delenv("EV2G_NO_BIG", raising=False)
    monkeypatch.delenv("EV2G_NO_FULL", raising=False)
    if no_big:
        monkeypatch.setenv("EV2G_NO_BIG", "1")
    eng = Engine(pool, 0, 0, device=0, flags=_abi.FLAG_LOG_SOC)
    monkeypatch.delenv("EV2G_NO_BIG", raising=False)
    assert eng.kernel_name == name and (eng.big_kernel_reason != "") == (C > 512 and no_big), (eng.kernel_name, eng.big_kernel_reason)
    P, D = eng.P, eng.D
    a64, o64 = eng.empty((k, E, P)).upload(acts.astype(np.float64)), eng.empty((k, E, D))
    rew, done, mask = eng.empty((k, E)), eng.empty((k, E), np.uint8), eng.empty((k, E, P), np.uint8)
    for strided, want in ((False, spec), (True, 0)):
        tag = f"{name} specialisation {want}"
        print(tag)
        eng.reset()
        s = (E * D, E, E, E * P) if strided else (0, 0, 0, 0)
        eng.step_n(k, a64, E * P, o64, s[0], rew, s[1], done, s[2], mask, s[3], auto_reset=False, persistent=True)
        assert eng.last_launch_specialisation == want, (tag, eng.last_launch_specialisation)
        got_o, got_r, got_d, got_m = o64.to_host(), rew.to_host(), done.to_host(), mask.to_host()
        for i, t in enumerate(range(k) if strided else [k - 1]):
            _close(got_o[i], ref["obs"][t], f"{tag}: obs[{t}]")
            _close(got_r[i], ref["reward"][t], f"{tag}: reward[{t}]")
            assert np.array_equal(got_d[i], ref["done"][t]) and np.array_equal(got_m[i], ref["mask"][t]), f"{tag}: done / mask [{t}]"
        check_state(eng, ref, tag, k)
    eng.close()
