"""The communication-fault link on the device (csrc/ev2g_link.h, ev2g_link_*; the reference's rl_agent/noise_wrappers.py): the kernels
against the reference's own wrapper objects (the link_* fixtures) and against the numpy model of ev2gym_amd.rl_agent.noise_wrappers (held to the
reference by tests/test_link_cpu.py), bit for bit, through every layer above them."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden
from tests.test_heuristics_gpu import DEFAULT_KINDS, PST_KINDS, _engine
from tests.test_link_cpu import LINK_FIXTURES, model_for

pytestmark = pytest.mark.gpu

P_HIT = 0.3
# (ports, envs, generator seed, link seed): the commands draw under `seed`, the observations under `seed + 1`; chosen on the CPU, where
# tests/test_link_cpu.py checks that every case has sessions and hits between a fifth and two fifths of its uniforms
LOCKSTEP = [(1, 1, 42, 5), (1, 5, 41, 10), (2, 1, 43, 3), (2, 5, 42, 6), (20, 1, 60, 3), (20, 5, 60, 3), (63, 1, 103, 3), (63, 5, 103, 3),
            (64, 1, 104, 3), (64, 5, 104, 3), (65, 1, 105, 3), (65, 5, 105, 3), (130, 1, 170, 3), (130, 5, 170, 3)]
GEN_SEED = {(P, E): g for P, E, g, _ in LOCKSTEP}


def lockstep_batch(P, E):
    """The generator's PublicPST kind with the charger count overridden, busy chargers, short episodes (longer for one or two ports: a
    share needs entries)."""
    from ev2gym_amd.scenario_gen import GenConfig, generate
    return generate(GenConfig.public_pst(E, P, seed=GEN_SEED[P, E], spawn_multiplier=10, simulation_length=48 if P >= 20 else 96))


def _same(a, b):
    """Bit for bit; an env without a departure has NaN statistics on both sides."""
    return np.array_equal(a, b, equal_nan=True)


def _uniforms(eng, seed):
    from ev2gym_amd.engine import host_uniform
    return host_uniform(eng.E * eng.P * eng.T, seed, 0.0, 1.0).reshape(eng.E, eng.P, eng.T)


def _bufs(eng, k):
    E, P, D = eng.E, eng.P, eng.D
    return dict(obs=eng.empty((k, E, D)), rew=eng.empty((k, E)), done=eng.empty((k, E), np.uint8), mask=eng.empty((k, E, P), np.uint8))


def _run(eng, link, k, agent=None, raw=None):
    """reset -> [delayed reset observation] -> link_run(k) with every step's outputs kept: obs [k + 1, E, D] (delivered), rew, done, mask,
    the raw actions [k, E, P] when an agent chose them, stats when the episode ended."""
    E, P, D = eng.E, eng.P, eng.D
    b, obs0 = _bufs(eng, k), eng.empty((E, D))
    eng.reset(obs0)
    if link is not None and link[1] > 0:
        eng.link_observe(link[0], obs0)
    act = eng.empty((k, E, P)) if raw is None else eng.empty((k, E, P)).upload(raw)
    if link is None:
        eng.step_n(k, act, E * P, b["obs"], E * D, b["rew"], E, b["done"], E, b["mask"], E * P, auto_reset=0, persistent=False)
    else:
        eng.link_run(link[0], k, agent, act, E * P, b["obs"], E * D, b["rew"], E, b["done"], E, b["mask"], E * P)
    out = {n: x.to_host() for n, x in b.items()}
    out["obs"] = np.concatenate([obs0.to_host()[None], out["obs"]])
    out["raw"] = act.to_host()
    if eng.current_step == eng.T:
        out["stats"] = eng.stats()
    eng.check_faults()
    for x in list(b.values()) + [obs0, act]:
        x.free()
    return out


def _model_run(eng, model, raw, k, delay=True):
    """The same episode by the model around plain per-step launches: delivered actions [k, E, P], delivered observations [k + 1, E, D], and
    the plain run they came from."""
    dlv = np.array([model.action(raw[t], t) for t in range(k)])
    plain = _run(eng, None, k, raw=dlv)
    obs = np.array([model.observation(plain["obs"][t], t) for t in range(k + 1)]) if delay else plain["obs"]
    return dlv, obs, plain


@pytest.mark.parametrize("tile", [1, 64])
@pytest.mark.parametrize("name", LINK_FIXTURES)
def test_device_reproduces_the_reference_wrappers_on_the_fixtures(name, tile):
    """The rows the reference's wrapper objects saw, through ev2g_link_actions / ev2g_link_observe with the wrapper's own matrix: the rows they
    delivered, bit for bit, and their float32 copies; then the whole episode through ev2g_link_run against the model around plain launches.
    64 envs: the fixture replicated, env 1 under another matrix (an env-index mix-up shows)."""
    z, batch, rk, sk = load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))
    eng = _engine(batch.tile(tile) if tile > 1 else batch, (str(z["case"][3]), str(z["case"][2])))
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    m = model_for(z, E)
    p_fail, p_delay = m.p_fail, m.p_delay
    if tile > 1:
        for r, seed in ((m.rand_act, 5), (m.rand_obs, 6)):
            if r is not None:
                r[1] = _uniforms(eng, seed)[1]
    link = eng.link_create(p_fail, p_delay, rand_act=m.rand_act, rand_obs=m.rand_obs)
    k = len(z["link_raw_act"])
    a_in, a_out, o, o32 = eng.empty((E, P)), eng.empty((E, P)), eng.empty((E, D)), eng.empty((E, D), np.float32)
    others = [e for e in range(E) if e != 1 or tile == 1]
    for t in range(k + 1):
        if p_delay:
            o.upload(np.tile(z["link_raw_obs"][t], (E, 1)))
            eng.link_observe(link, o, o32, t=t)
            got, want = o.to_host(), m.observation(np.tile(z["link_raw_obs"][t], (E, 1)), t)
            assert np.array_equal(got, want), (name, t)
            assert np.array_equal(got[others], np.tile(z["link_obs"][t], (len(others), 1))), (name, t)
            assert np.array_equal(o32.to_host(), np.float32(got))
        if p_fail and t < k:
            a_in.upload(np.tile(z["link_raw_act"][t], (E, 1)))
            eng.link_actions(link, a_in, a_out, t=t)
            got, want = a_out.to_host(), m.action(np.tile(z["link_raw_act"][t], (E, 1)), t)
            assert np.array_equal(got, want), (name, t)
            assert np.array_equal(got[others], np.tile(z["link_act"][t], (len(others), 1))), (name, t)
    eng.link_reset_state(link)
    m.reset_state()
    raw = np.tile(z["link_raw_act"][:, None, :], (1, E, 1))
    got = _run(eng, (link, p_delay), k, raw=raw)
    dlv, obs, plain = _model_run(eng, m, raw, k, delay=p_delay > 0)
    assert np.array_equal(got["obs"], obs) and np.array_equal(got["rew"], plain["rew"]) and np.array_equal(got["mask"], plain["mask"])
    ref = z["trj_obs"][1:k + 1]   # the delivered commands drive the reference's trajectory
    assert (np.abs(plain["obs"][1:, 0] - ref) / np.maximum(1.0, np.abs(ref))).max() <= 1e-9
    eng.close()


@pytest.mark.parametrize("P,E,gen_seed,seed", LOCKSTEP)
def test_randomised_lockstep_against_the_model(P, E, gen_seed, seed):
    """Whole episodes (the terminal observation included) under both halves at 0.3, uniforms generated on the device: the model around plain
    launches gives the same rows, and a link SUPPLIED with ev2g_host_uniform's matrix the same as the generating one."""
    eng = _engine(lockstep_batch(P, E), PST_KINDS)
    T = eng.T
    ua, uo = _uniforms(eng, seed), _uniforms(eng, seed + 1)
    raw = np.random.default_rng(seed).uniform(0, 1, (T, E, P))
    gen = eng.link_create(P_HIT, P_HIT, seed_act=seed, seed_obs=seed + 1)
    sup = eng.link_create(P_HIT, P_HIT, seed_act=99, seed_obs=98, rand_act=ua, rand_obs=uo)
    a, b = _run(eng, (gen, P_HIT), T, raw=raw), _run(eng, (sup, P_HIT), T, raw=raw)
    for n in ("obs", "rew", "mask", "stats"):
        assert _same(a[n], b[n]), n
    from ev2gym_amd.rl_agent.noise_wrappers import LinkModel
    m = LinkModel(E, P, T, eng.batch.timescale, P_HIT, P_HIT, ua, uo)
    dlv, obs, plain = _model_run(eng, m, raw, T)
    assert np.array_equal(a["obs"], obs) and np.array_equal(a["rew"], plain["rew"]) and _same(a["stats"], plain["stats"])
    held = (dlv != raw).mean()
    occ = plain["obs"][:T, :, 3::3] != 0
    late = ((uo < P_HIT).transpose(2, 0, 1) & occ).sum() / occ.sum()
    print(f"P={P} E={E}: held {held:.3f}, delayed {late:.3f} of {occ.sum()} occupied slot-steps, changed power readings "
          f"{(obs[:, :, 2] != plain['obs'][:, :, 2]).sum()}")
    assert 0.2 <= held <= 0.4 and 0.2 <= late <= 0.4
    assert np.array_equal(obs[T], np.where(np.arange(3 + 3 * P) == 2, np.maximum(plain["obs"][T], 0.0), plain["obs"][T]))   # terminal: through
    eng.close()


def test_directed_rows():
    """Synthetic rows through ev2g_link_observe / ev2g_link_actions, 130 slots (three chunks), every occupied slot delayed."""
    from ev2gym_amd.rl_agent.noise_wrappers import LinkModel
    eng = _engine(lockstep_batch(130, 1), PST_KINDS)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    zeros = np.zeros((E, P, T))
    link = eng.link_create(1.0, 1.0, rand_act=zeros, rand_obs=zeros)
    m = LinkModel(E, P, T, eng.batch.timescale, 1.0, 1.0, zeros, zeros)
    o, o32 = eng.empty((E, D)), eng.empty((E, D), np.float32)
    row = np.zeros((E, D))
    row[0, :3] = 0.25, 11.0, 7.0
    # two differences in slots 0..63, two in 64..127: in slot order ((1e16 + 1) - 1e16) + 1 = 1.0 (the first 1 is lost in 1e16, whose
    # spacing is 2); a partial per chunk gives 1e16 + (-1e16 + 1) = 0.0, and so does a tree over the four
    assert ((1e16 + 1.0) - 1e16) + 1.0 == 1.0 and (1e16 + 1.0) + (-1e16 + 1.0) == 0.0
    for i, d in ((3, 1e16), (40, 1.0), (70, -1e16), (100, 1.0)):
        row[0, 3 + 3 * i:6 + 3 * i] = 0.5, d, 2.0
    row[0, 4 + 3 * 5] = row[0, 4 + 3 * 129] = 123.0   # empty slots with a stale energy (first and third chunk): skipped, remembered as they are
    got = o.upload(row) and eng.link_observe(link, o, o32, t=1) or o.to_host()
    assert np.array_equal(got, m.observation(row, 1)) and got[0, 2] == 7.0 - 1.0 * 60 / eng.batch.timescale
    assert got[0, 4 + 3 * 5] == 123.0 and got[0, 4 + 3 * 129] == 123.0
    assert got[0, 4 + 3 * 3] == 0.0 and got[0, 4 + 3 * 100] == 0.0 and np.array_equal(o32.to_host(), np.float32(got))
    row2 = row.copy()
    row2[0, 2], row2[0, 4 + 3 * 40] = 1.0, 1000.0   # a small reading and much uncommunicated energy: clamped at 0, last
    got = o.upload(row2) and eng.link_observe(link, o, t=2) or o.to_host()
    assert np.array_equal(got, m.observation(row2, 2)) and got[0, 2] == 0.0 and got[0, 4 + 3 * 40] == 0.0 and got[0, 4 + 3 * 5] == 123.0
    got = o.upload(row) and eng.link_observe(link, o, t=T) or o.to_host()   # the terminal observation passes through
    assert np.array_equal(got, row) and np.array_equal(got, m.observation(row, T))
    got = o.upload(row2) and eng.link_observe(link, o, t=3) or o.to_host()   # ... and was remembered
    assert np.array_equal(got, m.observation(row2, 3)) and got[0, 4 + 3 * 40] == 1.0
    # float32 commands are widened exactly; p_fail = 1 holds the zeros for ever, p_fail = 0.3 mixes
    a32, out = eng.empty((E, P), np.float32), eng.empty((E, P))
    raw = np.random.default_rng(1).uniform(0, 1, (E, P)).astype(np.float32)
    eng.link_actions(link, a32.upload(raw), out, t=0, f32=True)
    assert not out.to_host().any()
    ua = _uniforms(eng, 8)
    mix = eng.link_create(P_HIT, 0.0, rand_act=ua)
    mm = LinkModel(E, P, T, eng.batch.timescale, P_HIT, 0.0, ua)
    for t in (0, 1, 2):
        raw = np.random.default_rng(t).uniform(0, 1, (E, P)).astype(np.float32)
        eng.link_actions(mix, a32.upload(raw), out, t=t, f32=True)
        want = mm.action(raw.astype(np.float64), t)
        assert np.array_equal(out.to_host(), want) and (t == 0 or 0 < (want != raw).sum() < P)
    eng.close()


def test_identities():
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.public_pst(8, 20, seed=6, spawn_multiplier=10, simulation_length=48))
    eng = _engine(batch, PST_KINDS)
    E, P, T = eng.E, eng.P, eng.T
    raw = np.random.default_rng(2).uniform(0, 1, (T, E, P))
    plain = _run(eng, None, T, raw=raw)
    off = _run(eng, (eng.link_create(0.0, 0.0), 0.0), T, raw=raw)   # both halves off: the per-step launches of step_n
    for n in ("obs", "rew", "done", "mask", "stats"):
        assert _same(off[n], plain[n]), n
    rr, link = eng.heuristic_create("RoundRobin"), eng.link_create(0.0, 0.0)
    b = _bufs(eng, T)
    act = eng.empty((T, E, P))
    eng.reset()
    eng.heuristic_run(rr, T, act, E * P, b["obs"], E * eng.D, b["rew"], E, b["done"], E, b["mask"], E * P)
    want = {n: x.to_host() for n, x in b.items()}
    want.update(raw=act.to_host(), stats=eng.stats())
    got = _run(eng, (link, 0.0), T, agent=rr)
    for n in ("raw", "rew", "done", "mask", "stats"):
        assert _same(got[n], want[n]), n
    assert np.array_equal(got["obs"][1:], want["obs"]) and want["raw"].any()
    nothing = _run(eng, None, T, raw=np.zeros((T, E, P)))   # p_fail = 1: the held zeros are held for ever -- DoNothing
    dead = _run(eng, (eng.link_create(1.0, 0.0, seed_act=4), 0.0), T, raw=raw)
    assert _same(dead["stats"], nothing["stats"]) and np.array_equal(dead["obs"], nothing["obs"])
    assert not _same(plain["stats"], nothing["stats"])
    frozen = _run(eng, (eng.link_create(0.0, 1.0, seed_obs=4), 1.0), T, raw=raw)   # p_delay = 1: an occupied slot shows what was shown before
    en, occ = frozen["obs"][:, :, 4::3], plain["obs"][:, :, 3::3] != 0
    assert np.array_equal(en[1:T][occ[1:T]], en[0:T - 1][occ[1:T]]) and occ[1:T].sum() > 100
    assert np.array_equal(en[T], plain["obs"][T, :, 4::3])   # the terminal row passes through
    eng.close()


def test_lifetime_and_refusals():
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.scenario_gen import GenConfig, generate
    eng = _engine(lockstep_batch(20, 5), PST_KINDS)
    E, P, T = eng.E, eng.P, eng.T
    raw = np.random.default_rng(3).uniform(0, 1, (T, E, P))
    link, fresh = eng.link_create(P_HIT, P_HIT, seed_act=1, seed_obs=2), eng.link_create(P_HIT, P_HIT, seed_act=1, seed_obs=2)
    first = _run(eng, (link, P_HIT), T, raw=raw)
    # the state carries over the reset, like the reference's objects: the first commands of the next episode meet the last ones held
    # (nobody is parked at step 0, so the episode's rows cannot show it: asked of the building block)
    act, out = eng.empty((E, P)).upload(raw[0]), eng.empty((E, P))
    eng.reset()
    eng.link_actions(link, act, out)
    carried = out.to_host()
    eng.link_actions(fresh, act, out)
    clean = out.to_host()
    hit = _uniforms(eng, 1)[:, :, 0] < P_HIT
    assert np.array_equal(carried[~hit], raw[0][~hit]) and np.array_equal(clean, np.where(hit, 0.0, raw[0])) and hit.sum() > 10
    assert (carried[hit] != 0).sum() > 10 and set(carried[hit]) <= set(raw.ravel())   # ... commands sent during the episode before
    eng.link_reset_state(link)
    eng.link_reset_state(fresh)
    third = _run(eng, (link, P_HIT), T, raw=raw)
    new = _run(eng, (fresh, P_HIT), T, raw=raw)
    for n in ("obs", "rew", "stats"):
        assert _same(third[n], first[n]) and _same(new[n], first[n]), n
    eng.reset()
    eng.link_run(link, T - 2, None, act)
    with pytest.raises(EngineError) as ei:
        eng.link_run(link, 3, None, act)                   # a segment that crosses the episode end
    assert ei.value.code == -4 and eng.current_step == T - 2
    eng.link_run(link, 2, None, act)
    for kw in (dict(p_fail=1.5), dict(p_delay=1.5), dict(p_fail=-0.1), dict(p_fail=float("nan"))):
        with pytest.raises(EngineError) as ei:
            eng.link_create(**kw)
        assert ei.value.code == -1
    eng.load(lockstep_batch(63, 5))                        # a reload that changes P: the link is refused from then on
    eng.reset()
    for call in (lambda: eng.link_run(link, 1, None, act), lambda: eng.link_actions(link, act), lambda: eng.link_reset_state(link)):
        with pytest.raises(EngineError) as ei:
            call()
        assert ei.value.code == -1 and "differ" in str(ei.value)
    assert eng.current_step == 0
    eng.close()
    v2g = _engine(generate(GenConfig.v2g_profit_plus_loads(4, 10, 1, seed=3)), DEFAULT_KINDS)
    with pytest.raises(EngineError) as ei:
        v2g.link_create(0.0, 0.3)                          # delayed observations on a V2G state
    assert ei.value.code == -1 and "PublicPST" in str(ei.value)
    ok = v2g.link_create(0.3, 0.0)
    with pytest.raises(EngineError) as ei:
        v2g.link_observe(ok, v2g.empty((v2g.E, v2g.D)))
    assert ei.value.code == -1
    v2g.close()


@pytest.mark.parametrize("name", ["ChargeAsLateAsPossible", "ChargeAsFastAsPossibleToDesiredCapacity", "RoundRobin",
                                  "ChargeAsLateAsPossibleToDesiredCapacity", "RoundRobin_GF", "RoundRobin_GF_off_allowed"])
def test_link_run_with_a_device_agent_equals_the_wrapped_facade_loop(name):
    """Per env: the facade agent on the single-env facade, its commands passed through the model before the step and the observation after
    it -- the device agent under ev2g_link_run chooses the same raw actions, delivers the same observations, ends with the same statistics."""
    from ev2gym_amd import _abi
    from ev2gym_amd.baselines import heuristics as H
    from ev2gym_amd.env import EV2Gym
    from ev2gym_amd.rl_agent.noise_wrappers import LinkModel
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.public_pst(3, 10, seed=21, spawn_multiplier=10, simulation_length=40, cs_min_charge_current=6.0,
                                          ev_desired_capacity=0.8))
    eng = _engine(batch, PST_KINDS)
    E, P, T = eng.E, eng.P, eng.T
    ua, uo = _uniforms(eng, 31), _uniforms(eng, 32)
    got = _run(eng, (eng.link_create(P_HIT, P_HIT, seed_act=31, seed_obs=32), P_HIT), T, agent=eng.heuristic_create(name))
    eng.close()
    assert got["raw"].any()
    for e in range(E):
        env = EV2Gym(scenario=batch.select([e]), state_function=PST_KINDS[1], reward_function=PST_KINDS[0])
        agent = getattr(H, name)(env=env)
        m = LinkModel(1, P, T, batch.timescale, P_HIT, P_HIT, ua[e:e + 1], uo[e:e + 1])
        obs, _ = env.reset()
        assert np.array_equal(m.observation(obs, 0)[0], got["obs"][0, e])
        for t in range(T):
            a = np.asarray(agent.get_action(env), np.float64)
            assert np.array_equal(a, got["raw"][t, e]), (name, e, t)
            obs = env.step(m.action(a, t)[0])[0]
            assert np.array_equal(m.observation(obs, t + 1)[0], got["obs"][t + 1, e]), (name, e, t)
        for i, k in enumerate(_abi.STAT_NAMES):
            g, w = float(got["stats"][e, i]), float(env.stats[k])
            assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= 1e-9 * max(1.0, abs(w)), (name, e, k, g, w)
        env.close()


@pytest.mark.parametrize("p_delay", [P_HIT, 0.0])
def test_link_rollout_equals_the_loop_of_its_parts(p_delay):
    from ev2gym_amd.actor import init_mlp_weights
    eng = _engine(lockstep_batch(20, 5), PST_KINDS)
    E, P, D, T = eng.E, eng.P, eng.D, eng.T
    mlp = eng.mlp_create(*init_mlp_weights(D, P, seed=9), out_lo=0.0)
    rew, done, mask = eng.empty((T, E)), eng.empty((T, E), np.uint8), eng.empty((T, E, P), np.uint8)
    obs = eng.empty((E, D))
    link = eng.link_create(P_HIT, p_delay, seed_act=5, seed_obs=6)
    o32 = eng.link_obs_f32(link)
    eng.reset(obs)
    eng.link_observe(link, obs, o32, t=0)
    eng.link_rollout(link, mlp, T // 2, rew, E, done, E, mask, E * P)
    eng.link_rollout(link, mlp, T - T // 2, rew.at(T // 2 * E), E, done.at(T // 2 * E), E, mask.at(T // 2 * E * P), E * P)
    got = dict(rew=rew.to_host(), done=done.to_host(), mask=mask.to_host(), stats=eng.stats())
    from ev2gym_amd.engine import EngineError
    with pytest.raises(EngineError) as ei:
        eng.link_rollout(link, mlp, 1, rew, E, done, E, mask, E * P)
    assert ei.value.code == -4
    # the same chain from the test's side, a fresh link
    link = eng.link_create(P_HIT, p_delay, seed_act=5, seed_obs=6)
    x32, a32, dlv = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32), eng.empty((E, P))
    r1, d1, m1 = eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    eng.reset(obs)
    eng.link_observe(link, obs, x32, t=0)
    held = 0
    for t in range(T):
        eng.mlp_forward(mlp, x32, a32, E)
        eng.link_actions(link, a32, dlv, f32=True)
        held += int((dlv.to_host() != a32.to_host().astype(np.float64)).sum())
        eng.step(dlv, obs, r1, d1, m1)
        eng.link_observe(link, obs, x32)   # (p_delay = 0: nothing is delayed, the float32 copy is written)
        assert np.array_equal(got["rew"][t], r1.to_host()) and np.array_equal(got["mask"][t], m1.to_host()), t
        assert np.array_equal(got["done"][t], d1.to_host())
    assert _same(got["stats"], eng.stats()) and 0.2 <= held / (T * E * P) <= 0.4 and got["mask"].any()
    eng.close()


def test_evaluate_under_failed_commands_equals_the_link_run_loops():
    from ev2gym_amd import _abi
    from ev2gym_amd.evaluator import ALGORITHMS, RESULT_STATS, evaluate
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.v2g_profit_plus_loads(8, 10, 1, seed=9, power_setpoint_enabled=True, simulation_length=48))
    E, T, P = batch.n_envs, batch.n_steps, batch.n_ports
    names = list(ALGORITHMS) + ["RoundRobin", "ChargeAsLateAsPossible"]
    df = evaluate(batch, algorithms=names, seed=3, p_fail=P_HIT, fail_seed=11)
    assert len(df) == E * len(names) and (df["time"] > 0).all()
    idx = {n: i for i, n in enumerate(_abi.STAT_NAMES)}
    tables = {}
    for name in names:
        eng = _engine(batch, DEFAULT_KINDS)
        link = eng.link_create(P_HIT, 0.0, seed_act=11)
        eng.reset()
        if name in ALGORITHMS:
            raw = {"ChargeAsFastAsPossible": np.ones((T, E, P)), "DoNothing": np.zeros((T, E, P))}.get(name)
            act = eng.empty((T, E, P))
            if raw is None:
                eng.fill_uniform(act, T * E * P, 3, -1.0 if batch.v2g_enabled else 0.0, 1.0)
            else:
                act.upload(raw)
            eng.link_run(link, T, None, act, E * P)
        else:
            eng.link_run(link, T, eng.heuristic_create(name))
        tables[name] = eng.stats()
        eng.close()
        sub = df[df["Algorithm"] == name].sort_values("run")
        for k in RESULT_STATS + ["total_reward"]:
            assert np.array_equal(sub[k].to_numpy(), tables[name][:, idx[k]], equal_nan=True), (name, k)
    assert not _same(tables["ChargeAsFastAsPossible"], tables["RandomAgent"])
    plain, again = evaluate(batch, algorithms=names, seed=3), evaluate(batch, algorithms=names, seed=3, p_fail=0.0)
    cols = RESULT_STATS + ["total_reward"]
    assert np.array_equal(plain[cols].to_numpy(), again[cols].to_numpy(), equal_nan=True)
    assert not np.array_equal(plain[cols].to_numpy(), df[cols].to_numpy(), equal_nan=True)
    eng = _engine(batch, DEFAULT_KINDS)   # the default call: today's table (a persistent launch of constant commands)
    eng.reset()
    eng.step_n(T, eng.empty((E, P)).upload(np.ones((E, P))), 0, auto_reset=0, persistent=True)
    st = eng.stats()
    eng.close()
    sub = plain[plain["Algorithm"] == "ChargeAsFastAsPossible"].sort_values("run")
    for k in cols:
        assert np.array_equal(sub[k].to_numpy(), st[:, idx[k]], equal_nan=True), k


def test_wrappers_on_the_vector_env_and_the_facade():
    """DelayedObservation(FailedActionCommunication(env)) on an EV2GymVec (numpy hand-over) and on the single-env facade: the rows and rewards
    of ev2g_link_run on the same scenarios under the same seeds."""
    from ev2gym_amd.env import EV2Gym
    from ev2gym_amd.rl_agent.noise_wrappers import DelayedObservation, FailedActionCommunication
    from ev2gym_amd.vec_env import EV2GymVec
    batch = lockstep_batch(20, 5)
    eng = _engine(batch, PST_KINDS)
    E, P, T = eng.E, eng.P, eng.T
    raw = np.random.default_rng(4).uniform(0, 1, (T, E, P))
    want = _run(eng, (eng.link_create(P_HIT, P_HIT, seed_act=7, seed_obs=8), P_HIT), T, raw=raw)
    ua, uo = _uniforms(eng, 7), _uniforms(eng, 8)
    eng.close()
    vec = EV2GymVec(scenarios=batch, num_envs=E, state_function=PST_KINDS[1], reward_function=PST_KINDS[0], auto_reset=False, use_torch=False)
    env = DelayedObservation(FailedActionCommunication(vec, P_HIT, seed=7), P_HIT, seed=8)
    assert env.unwrapped is vec and env.simulation_length == T and np.array_equal(env.random, uo) and np.array_equal(env.env.random, ua)
    obs, _ = env.reset(seed=0)
    assert vec.engine.scenario_offset == 0 and np.array_equal(obs, want["obs"][0])
    for t in range(T):
        obs, rew, done, _, info = env.step(raw[t])
        assert np.array_equal(obs, want["obs"][t + 1]) and np.array_equal(rew, want["rew"][t]), t
    assert done.all()
    env.close()
    one = EV2Gym(scenario=batch.select([2]), state_function=PST_KINDS[1], reward_function=PST_KINDS[0])
    env = DelayedObservation(FailedActionCommunication(one, P_HIT, random=ua[2]), P_HIT, random=uo[2])
    obs, _ = env.reset()
    assert np.array_equal(obs, want["obs"][0, 2])
    for t in range(T):
        obs, rew, done, _, info = env.step(raw[t, 2].copy())
        assert np.array_equal(obs, want["obs"][t + 1, 2]) and rew == want["rew"][t, 2], t
    assert done
    env.close()


def test_wrappers_on_the_vector_env_with_the_torch_hand_over():
    """The same stack on an EV2GymVec that hands torch tensors over (the engine on torch's stream, the kernels on the tensors' memory): device
    actions in, device rows out, bit for bit ev2g_link_run's; a wrapper whose link was destroyed refuses to step."""
    import torch
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.rl_agent.noise_wrappers import DelayedObservation, FailedActionCommunication
    from ev2gym_amd.vec_env import EV2GymVec
    batch = lockstep_batch(20, 5)
    eng = _engine(batch, PST_KINDS)
    E, P, T = eng.E, eng.P, eng.T
    raw = np.random.default_rng(4).uniform(0, 1, (T, E, P))
    want = _run(eng, (eng.link_create(P_HIT, P_HIT, seed_act=7, seed_obs=8), P_HIT), T, raw=raw)
    eng.close()
    vec = EV2GymVec(scenarios=batch, num_envs=E, state_function=PST_KINDS[1], reward_function=PST_KINDS[0], auto_reset=False, use_torch=True)
    env = DelayedObservation(FailedActionCommunication(vec, P_HIT, seed=7), P_HIT, seed=8)
    acts = torch.from_numpy(raw).to("cuda:0")
    obs, _ = env.reset(seed=0)
    assert torch.is_tensor(obs) and obs.is_cuda and np.array_equal(obs.cpu().numpy(), want["obs"][0])
    for t in range(T):
        obs, rew, done, _, info = env.step(acts[t] if t % 2 else raw[t])   # a device tensor, or a host array copied into the env's buffer
        assert obs.is_cuda and np.array_equal(obs.cpu().numpy(), want["obs"][t + 1]) and np.array_equal(rew.cpu().numpy(), want["rew"][t]), t
    assert bool(done.all()) and np.array_equal(acts.cpu().numpy(), raw)   # the caller's tensors are not written
    env.reset(seed=0)
    env.env.destroy_link()
    with pytest.raises(EngineError) as ei:
        env.step(acts[0])
    assert ei.value.code == -1
    env.close()
