"""CPU side of the communication-fault link (csrc/ev2g_link.h, ev2g_link_*; the reference's rl_agent/noise_wrappers.py): the numpy model of
both wrappers against the link_* fixtures (recorded from the reference's own wrapper objects) and against the live reference where a
checkout exists, the C-ABI surface, the kernels' register budget, the evaluator's dispatch and refusals on a stand-in engine."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT

LINK_FIXTURES = ("link_fail_v2gppl_s81", "link_fail_pst_s82", "link_delay_pst_s83", "link_both_pst_s84")
LINK_SYMBOLS = ("ev2g_link_create", "ev2g_link_destroy", "ev2g_link_reset_state", "ev2g_link_actions", "ev2g_link_observe", "ev2g_link_obs_f32",
                "ev2g_link_run", "ev2g_link_rollout")


def model_for(z, E=1):
    """LinkModel of a fixture: its probabilities and the wrapper's recorded uniforms, for E copies of the env."""
    from ev2gym_amd.rl_agent.noise_wrappers import LinkModel
    p_fail, p_delay = (float(x) for x in z["link_p"])
    from ev2gym_amd.scenario import ScenarioBatch
    batch = ScenarioBatch.from_single(z)
    T, P = batch.n_steps, batch.n_ports
    tile = lambda r: np.broadcast_to(r, (E,) + r.shape).copy() if r.size else None   # noqa: E731
    return LinkModel(E, P, T, batch.timescale, p_fail, p_delay, tile(z["link_rand_act"]), tile(z["link_rand_obs"]))


def test_the_fixtures_are_in_place_and_hit_a_quarter_to_a_third():
    assert sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("link_")) == sorted(LINK_FIXTURES)
    for name in LINK_FIXTURES:
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        assert os.path.getsize(path) < 1 << 20
        z = np.load(path)
        p_fail, p_delay = z["link_p"]
        assert np.array_equal(z["act"], z["link_act"]) and np.array_equal(z["trj_obs"], z["link_raw_obs"])
        if p_fail:
            assert p_fail == 0.3 and 0.25 <= (z["link_act"] != z["link_raw_act"]).mean() <= 0.35
        else:
            assert np.array_equal(z["link_act"], z["link_raw_act"])
        if p_delay:
            assert p_delay == 0.3 and str(z["case"][2]) == "PublicPST" and len(z["link_obs"]) == z["scn_power_setpoints"].shape[-1]   # T - 1 steps
            occupied = z["link_raw_obs"][:, 3::3] != 0
            late = (z["link_obs"] != z["link_raw_obs"])[:, 4::3]
            hit = occupied & (z["link_rand_obs"].T[:len(occupied)] < p_delay)   # (a delayed column may equal the raw one: the EV idled)
            assert not late[~hit].any() and late.sum() >= 50 and 0.25 <= hit.sum() / occupied.sum() <= 0.35
            assert (z["link_obs"][:, 2] != z["link_raw_obs"][:, 2]).sum() > 10
        else:
            assert np.array_equal(z["link_obs"], z["link_raw_obs"])


@pytest.mark.parametrize("name", LINK_FIXTURES)
def test_numpy_model_reproduces_the_reference_wrappers_on_the_fixtures(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    m = model_for(z)
    pst = str(z["case"][2]) == "PublicPST"   # (the model's observation half has the wrapper's layout assertion)
    assert not pst or np.array_equal(m.observation(z["link_raw_obs"][0], 0)[0], z["link_obs"][0])
    for t in range(len(z["link_raw_act"])):
        assert np.array_equal(m.action(z["link_raw_act"][t], t)[0], z["link_act"][t]), (name, t)
        assert not pst or np.array_equal(m.observation(z["link_raw_obs"][t + 1], t + 1)[0], z["link_obs"][t + 1]), (name, t)


def test_numpy_model_edges():
    """The clamp comes last, empty slots are skipped whatever stale energy they carry, the sum runs in slot order, the terminal row passes."""
    from ev2gym_amd.rl_agent.noise_wrappers import LinkModel
    P, T = 130, 4
    m = LinkModel(1, P, T, 15, 0.0, 1.0, None, np.zeros((1, P, T)))
    row = np.zeros(3 + 3 * P)
    row[2] = 7.0
    for i, d in ((3, 1e16), (40, 1.0), (70, -1e16), (100, 1.0)):   # two per 64-slot chunk: a partial per chunk, or a tree, sums them to 0.0
        row[3 + 3 * i], row[4 + 3 * i] = 0.5, d
    row[4 + 3 * 5] = row[4 + 3 * 129] = 123.0   # empty slots with stale energy
    out = m.observation(row, 1)[0]
    nc = ((1e16 + 1.0) - 1e16) + 1.0
    assert nc == 1.0 and (1e16 + 1.0) + (-1e16 + 1.0) == 0.0
    assert out[2] == 7.0 - nc * 60 / 15 and out[4 + 3 * 5] == 123.0 and out[4 + 3 * 129] == 123.0 and out[4 + 3 * 3] == 0.0 and out[4 + 3 * 100] == 0.0
    assert np.array_equal(m.actual[0, [3, 5, 40]], [1e16, 123.0, 1.0]) and m.prev[0, 3] == 0.0 and m.prev[0, 5] == 123.0
    row2 = row.copy()
    row2[2], row2[4 + 3 * 40] = 1.0, 1000.0
    assert m.observation(row2, 2)[0][2] == 0.0   # 1 - 999 * 4 clamped
    term = m.observation(row, T)[0]
    assert np.array_equal(term, row)
    f = LinkModel(2, 3, T, 15, 1.0, 0.0, np.zeros((2, 3, T)))
    assert not f.action(np.ones((2, 3)), 0).any() and not f.action(np.ones((2, 3)), 1).any()   # held zeros are held forever


_LIVE = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1] + "/tools"); sys.path.insert(1, sys.argv[1])
import capture_link_fixtures as cl
cl.import_reference()
cg = cl.cg
from ev2gym.models.ev2gym_env import EV2Gym
import ev2gym.rl_agent.noise_wrappers as NW
import ev2gym.rl_agent.reward as RW
import ev2gym.rl_agent.state as S
from ev2gym_amd.rl_agent.noise_wrappers import LinkModel
cfg = cg._yaml_variant("ev2gym/example_config_files/PublicPST.yaml", {"simulation_length": 40, "spawn_multiplier": 10}, "link_live")
for seed in (91, 92):
    env = EV2Gym(config_file=cfg, seed=seed, state_function=S.PublicPST, reward_function=RW.SquaredTrackingErrorReward, generate_rnd_game=True)
    np.random.seed(seed)
    fail, delay = NW.FailedActionCommunication(env, p_fail=0.3), NW.DelayedObservation(env, p_delay=0.3)
    P, T = env.number_of_ports, env.simulation_length
    m = LinkModel(1, P, T, env.timescale, 0.3, 0.3, fail.random[None], delay.random[None])
    rng = np.random.default_rng(seed)
    late = 0
    for episode in range(2):   # the wrappers' state carries over the reset
        obs, _ = env.reset(seed=seed + episode)
        assert np.array_equal(m.observation(obs.copy(), 0)[0], delay.observation(obs.copy()))
        for t in range(T - 1):   # (the reference raises at the terminal observation)
            a = rng.uniform(0, 1, P)
            d = fail.action(a)
            assert np.array_equal(m.action(a, t)[0], d), (seed, episode, t)
            obs = env.step(d.copy())[0]
            mine, ref = m.observation(obs.copy(), t + 1)[0], delay.observation(obs.copy())
            assert np.array_equal(mine, ref), (seed, episode, t, mine - ref)
            late += int((ref != obs).sum())
    assert late > 20, late
print("OK")
"""


def test_numpy_model_equals_the_live_reference_wrappers(tmp_path):
    """Two short reference episodes per seed through the reference's own wrapper objects, the model in lockstep, bit for bit.  Needs a checkout
    of the upstream reference (not part of this repository); in its own process because the import shim installs module stubs and changes
    the working directory."""
    from oracle.ref_import import REF_ROOT
    if not os.path.isdir(os.path.join(REF_ROOT, "ev2gym")):
        pytest.skip(f"no checkout of the upstream reference at {REF_ROOT} (not part of this repository)")
    r = subprocess.run([sys.executable, "-c", _LIVE, ROOT], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-1500:], r.stderr[-3000:])


def test_link_symbols_are_declared_exported_and_bound():
    import ctypes
    from ev2gym_amd import build, engine
    txt = open(os.path.join(ROOT, "include", "ev2g.h")).read()
    L = ctypes.CDLL(build.build())
    for name in LINK_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(L, name) and name in engine.EXPORTED_SYMBOLS
        assert hasattr(engine.Engine, name[len("ev2g_"):]), name
    assert re.search(r"#define EV2G_ABI_VERSION\s+4\b", txt)   # additive: the ABI version stays
    for words in ("passes through with no slot delayed", "is not reproduced", "NO\n * fused-launch variant"):
        assert words in txt, words


def test_link_kernels_compile_without_spills_or_scratch(tmp_path):
    """The compiler's own figures (-Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950) for the three kernels of ev2g_link.h."""
    from ev2gym_amd import build
    src = tmp_path / "link.hip"
    src.write_text('#include "ev2g_link.h"\n'
                   "template __global__ void ev2g_link_act_kernel<false>(const void *, LinkRand, double, int, double *, double *);\n"
                   "template __global__ void ev2g_link_act_kernel<true>(const void *, LinkRand, double, int, double *, double *);\n")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-I", os.path.join(ROOT, "ev2gym_amd", "csrc"), "--cuda-device-only", "-c",
                                     "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, str(src)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur:
            res.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    link = {k: v for k, v in res.items() if "ev2g_link_" in k}
    assert len(link) == 4, sorted(res)   # act<false>, act<true>, obs, f32
    for k, v in link.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)


class _Engine:
    """Stand-in for ev2gym_amd.engine.Engine with the calls evaluate(p_fail=...) makes, recording them."""
    calls = []

    def __init__(self, batch, rk, sk):
        self.E, self.T, self.P = batch.n_envs, batch.n_steps, batch.n_ports

    def link_create(self, p_fail=0.0, p_delay=0.0, seed_act=0, seed_obs=0, rand_act=None, rand_obs=None):
        if not (0 <= p_fail <= 1 and 0 <= p_delay <= 1):   # EV2G_ERR_ARG of ev2g_link_create
            raise ValueError("probability")
        self.calls.append(("link", p_fail, p_delay, seed_act))
        return "link"

    def heuristic_create(self, name):
        self.calls.append(("agent", name))
        return name

    def empty(self, shape, dtype=np.float64):
        class Buf:
            def upload(self, a):
                self.value = float(np.asarray(a).flat[0])
                return self
        b = Buf()
        b.shape = shape
        return b

    def fill_uniform(self, dst, n, seed, lo, hi):
        self.calls.append(("uniform", n, seed, lo, hi))

    def reset(self):
        self.calls.append(("reset",))

    def link_run(self, link, k, agent=None, actions=None, a_stride=0):
        self.calls.append(("run", link, k, agent, None if actions is None else (actions.shape, getattr(actions, "value", None)), a_stride))

    def step_n(self, *a, **k):
        self.calls.append(("step_n",))

    def stats(self):
        from ev2gym_amd import _abi
        return np.zeros((self.E, _abi.N_STATS))

    def check_faults(self):
        pass

    def last_step_n_kernel_ms(self):
        return 2.0

    def close(self):
        pass


def test_evaluate_routes_every_algorithm_through_link_run_and_refuses_what_it_cannot_do():
    from ev2gym_amd.evaluator import ALGORITHMS, evaluate
    from ev2gym_amd.scenario_gen import GenConfig, generate
    batch = generate(GenConfig.v2g_profit_plus_loads(3, 6, 1, seed=4))
    E, T, P = batch.n_envs, batch.n_steps, batch.n_ports
    assert evaluate.__defaults__[0] == ALGORITHMS and evaluate.__defaults__[-2:] == (0.0, 0)
    _Engine.calls = []
    names = ["ChargeAsFastAsPossible", "DoNothing", "RandomAgent", "RoundRobin"]
    df = evaluate(batch, algorithms=names, engine_factory=_Engine, p_fail=0.3, fail_seed=7, seed=5)
    assert len(df) == E * len(names)
    lo = -1.0 if batch.v2g_enabled else 0.0
    assert _Engine.calls == [
        ("link", 0.3, 0.0, 7), ("reset",), ("run", "link", T, None, ((E, P), 1.0), 0),
        ("link", 0.3, 0.0, 7), ("reset",), ("run", "link", T, None, ((E, P), 0.0), 0),
        ("link", 0.3, 0.0, 7), ("uniform", T * E * P, 5, lo, 1.0), ("reset",), ("run", "link", T, None, ((T, E, P), None), E * P),
        ("link", 0.3, 0.0, 7), ("agent", "RoundRobin"), ("reset",), ("run", "link", T, "RoundRobin", None, 0)]
    _Engine.calls = []
    evaluate(batch, algorithms=["DoNothing"], engine_factory=_Engine)   # the default: today's path, no link
    assert _Engine.calls == [("reset",), ("step_n",)]
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            evaluate(batch, algorithms=["DoNothing"], engine_factory=_Engine, p_fail=bad)

    class _Bare:
        def __init__(self, *a):
            pass

        def close(self):
            pass

    with pytest.raises(NotImplementedError):
        evaluate(batch, algorithms=["DoNothing"], engine_factory=_Bare, p_fail=0.3)


def test_wrappers_refuse_an_engine_without_links():
    from ev2gym_amd.rl_agent import noise_wrappers as NW

    class _Env:
        num_envs = 2

        class engine:
            E, P, T = 2, 3, 4

    for cls in (NW.FailedActionCommunication, NW.DelayedObservation):
        with pytest.raises(NotImplementedError) as ei:
            cls(_Env(), 0.3)
        assert "link_" in str(ei.value)


def test_wrappers_destroy_their_links_on_close():
    """A wrapper's link goes with the wrapper: close() destroys each link of a stack once, then closes the env; destroy_link() leaves the env
    open for the next wrapper (the caller who wraps one env anew per run)."""
    from ev2gym_amd.rl_agent import noise_wrappers as NW
    log = []

    class _Eng:
        E, P, T = 2, 3, 4

        def link_create(self, p_fail=0.0, p_delay=0.0, **kw):
            log.append(("create", p_fail, p_delay))
            return len(log)

        def link_destroy(self, link):
            log.append(("destroy", link))

    class _Env:
        num_envs = 2
        engine = _Eng()

        def close(self):
            log.append(("close",))

    env = _Env()
    for run in range(3):   # re-wrapped per run: no link outlives its wrapper
        w = NW.FailedActionCommunication(env, 0.3)
        w.destroy_link()
        w.destroy_link()
    assert log == [("create", 0.3, 0.0), ("destroy", 1), ("create", 0.3, 0.0), ("destroy", 3), ("create", 0.3, 0.0), ("destroy", 5)]
    del log[:]
    NW.DelayedObservation(NW.FailedActionCommunication(env, 0.3), 0.2).close()
    assert log == [("create", 0.3, 0.0), ("create", 0.0, 0.2), ("destroy", 2), ("destroy", 1), ("close",)]


def test_the_lockstep_cases_hit_a_fifth_to_two_fifths_of_the_uniforms():
    """tests/test_link_gpu.py's randomised cases, checked here with the generator alone: under each case's seeds between 0.2 and 0.4 of the
    uniforms are below 0.3, for the commands and -- over the slot-steps a session covers -- for the observations."""
    from ev2gym_amd.engine import host_uniform
    from ev2gym_amd.scenario import resolve_ports
    from tests.test_link_gpu import LOCKSTEP, lockstep_batch
    for P, E, _, seed in LOCKSTEP:
        batch = lockstep_batch(P, E)
        T = batch.n_steps
        assert batch.n_ports == P and batch.n_envs == E
        ua = host_uniform(E * P * T, seed, 0.0, 1.0).reshape(E, P, T)
        uo = host_uniform(E * P * T, seed + 1, 0.0, 1.0).reshape(E, P, T)
        assert 0.2 <= (ua < 0.3).mean() <= 0.4, (P, E, seed, (ua < 0.3).mean())
        a, port = batch.arrays, resolve_ports(batch)
        occ = np.zeros((E, P, T), bool)
        for e in range(E):
            for s in range(int(a["env_session_start"][e]), int(a["env_session_start"][e + 1])):
                if port[s] >= 0:
                    occ[e, port[s], max(int(a["ev_t_arr"][s]), 0):min(int(a["ev_t_dep"][s]), T - 1) + 1] = True
        assert occ.sum() >= 40, (P, E, occ.sum())
        share = (uo < 0.3)[occ].mean()
        assert 0.22 <= share <= 0.38, (P, E, seed, share, occ.sum())
