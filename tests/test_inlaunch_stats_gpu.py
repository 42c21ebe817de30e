"""Episode statistics computed inside the step launch that closes the episode (ev2g_step_wave's in-launch phase): bit-identical to the
statistics kernel, and the routing between the two (ev2g_last_stats_route / ev2g_last_stats_reason) across every transition that must fall
back to the statistics kernel.  Every comparison is against a second engine loaded with EV2G_NO_INLAUNCH_STATS=1 and driven identically."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _engines(batch, rk, sk, flags, monkeypatch, n_active=0):
    """(engine with in-launch statistics, engine with the statistics kernel only) over the same batch."""
    from ev2gym_amd.engine import Engine
    monkeypatch.setenv("EV2G_NO_INLAUNCH_STATS", "1")
    ref = Engine(batch, rk, sk, device=0, flags=flags, n_active_envs=n_active)
    monkeypatch.delenv("EV2G_NO_INLAUNCH_STATS")
    eng = Engine(batch, rk, sk, device=0, flags=flags, n_active_envs=n_active)
    return eng, ref


class _Run:
    """Device buffers of one engine and the same uniform action block for every episode."""

    def __init__(self, eng, lo, seed):
        E, P, D, T = eng.E, eng.P, eng.D, eng.T
        self.eng, self.E, self.P, self.T = eng, E, P, T
        self.acts = eng.empty((T, E, P))
        eng.fill_uniform(self.acts, T * E * P, seed, lo, 1.0)
        self.obs, self.rew = eng.empty((E, D)), eng.empty((E,))
        self.done, self.mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
        self.out = eng.empty((E, 17))

    def steps(self, k, persistent=True):
        t = self.eng.current_step
        self.eng.step_n(k, self.acts.at(t * self.E * self.P), self.E * self.P, self.obs, 0, self.rew, 0, self.done, 0, self.mask, 0,
                        auto_reset=False, persistent=persistent)

    def stats(self):
        return self.eng.stats()

    def stats_reset(self, offset):
        self.eng.stats_reset(self.out, self.obs, offset)
        return self.out.to_host().copy(), self.obs.to_host().copy()


def _same(a, b, what):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)   # (NaN == NaN here: bit-identical rows)


def _workload(name, E, seed):
    from bench import WORKLOADS
    from ev2gym_amd import _abi
    from ev2gym_amd.scenario_gen import generate_native
    wl = WORKLOADS[name]
    batch = generate_native(wl["gen"](2 * E, seed))
    return batch, _abi.REWARD_KINDS[wl["reward"]], _abi.STATE_KINDS[wl["state"]], wl["lo"]


@pytest.mark.parametrize("seed", [3, 41])
@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_whole_episodes_bit_identical_to_the_statistics_kernel(name, seed, monkeypatch):
    """Three whole episodes (one persistent launch each) over two pool windows: stats() and stats_reset() of the in-launch engine equal the
    statistics kernel's bit for bit, and so does the reset observation.  cfg2 (one env per wavefront) takes the in-launch route; cfg3 (three
    envs per wavefront) keeps the statistics kernel and says why."""
    from ev2gym_amd import _abi
    E = 512 if name == "cfg2" else 768
    batch, rk, sk, lo = _workload(name, E, seed)
    eng, ref = _engines(batch, rk, sk, _abi.FLAG_LOG_SOC, monkeypatch, n_active=E)
    a, b = _Run(eng, lo, 100 + seed), _Run(ref, lo, 100 + seed)
    inl = name == "cfg2"
    for x in (a, b):
        x.eng.reset(x.obs, offset=0)
    for ep in range(3):
        for x in (a, b):
            x.steps(x.T)
        assert eng.last_launch_specialisation == 2
        _same(a.stats(), b.stats(), f"{name} episode {ep}: stats()")
        assert eng.last_stats_route == (1 if inl else 0), (eng.last_stats_route, eng.last_stats_reason)
        assert ref.last_stats_route == 0 and "EV2G_NO_INLAUNCH_STATS" in ref.last_stats_reason
        if not inl:
            assert "several envs per wavefront" in eng.last_stats_reason
        _same(a.stats(), b.stats(), f"{name} episode {ep}: stats() twice")
        (sa, oa), (sb, ob) = a.stats_reset(((ep + 1) % 2) * E), b.stats_reset(((ep + 1) % 2) * E)
        assert eng.last_stats_route == (1 if inl else 0)
        _same(sa, sb, f"{name} episode {ep}: stats_reset()")
        _same(oa, ob, f"{name} episode {ep}: reset observation")
        assert np.isfinite(sa[:, 0]).all()
    eng.check_faults()
    eng.close(); ref.close()


def test_fallback_transitions(monkeypatch):
    """A mid-episode stats(), an episode whose first half ran per-step launches and whose second half ran one persistent launch, one whose
    last step was a single-step launch, and a reset: each time the route is the one the state allows, and the values equal the kernel's."""
    from ev2gym_amd import _abi
    E = 256
    batch, rk, sk, lo = _workload("cfg2", E, 7)
    eng, ref = _engines(batch, rk, sk, _abi.FLAG_LOG_SOC, monkeypatch, n_active=E)
    a, b = _Run(eng, lo, 5), _Run(ref, lo, 5)
    T = a.T
    for x in (a, b):
        x.eng.reset(x.obs)
        x.steps(40)
    _same(a.stats(), b.stats(), "mid-episode")
    assert eng.last_stats_route == 0 and "did not end the episode" in eng.last_stats_reason
    for x in (a, b):
        x.steps(T - 40)
    _same(a.stats(), b.stats(), "second launch closes the episode")
    assert eng.last_stats_route == 1 and eng.last_stats_reason == ""
    # per-step launches, then one persistent launch to the end
    (sa, _), (sb, _) = a.stats_reset(E), b.stats_reset(E)
    _same(sa, sb, "stats_reset after a split episode")
    for x in (a, b):
        x.steps(60, persistent=False)
    _same(a.stats(), b.stats(), "after per-step launches")
    assert eng.last_stats_route == 0
    for x in (a, b):
        x.steps(T - 60)
    _same(a.stats(), b.stats(), "per_step -> persistent")
    assert eng.last_stats_route == 1
    # a persistent launch, then the episode's last step as a single-step launch
    for x in (a, b):
        x.eng.reset(x.obs, offset=0)
        x.steps(T - 1)
        x.steps(1, persistent=False)
    _same(a.stats(), b.stats(), "persistent -> per_step")
    assert eng.last_stats_route == 0 and "single-step launch" in eng.last_stats_reason
    # the in-launch results belong to the episode that produced them: a reset discards them
    for x in (a, b):
        x.eng.reset(x.obs, offset=0)
        x.steps(T)
        x.eng.reset(x.obs, offset=E)
    _same(a.stats(), b.stats(), "after a reset")
    assert eng.last_stats_route == 0 and "reset" in eng.last_stats_reason
    eng.close(); ref.close()


def test_refill_between_episodes(monkeypatch):
    """Device refills of the pool between episodes (the refill benchmark's loop: statistics and reset onto the next window, then a refill of
    the window before); a refill between an episode's last launch and its statistics sends them back to the statistics kernel."""
    from ev2gym_amd import _abi
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    E = 128
    cfg = GenConfig.v2g_profit_plus_loads(3 * E, 50, 1, seed=19)
    rk, sk = _abi.REWARD_KINDS["ProfitMax_TrPenalty_UserIncentives"], _abi.STATE_KINDS["V2G_profit_max_loads"]
    eng, ref = _engines(generate_native(cfg), rk, sk, _abi.FLAG_LOG_SOC | _abi.FLAG_REFILLABLE, monkeypatch, n_active=E)
    a, b = _Run(eng, -1.0, 9), _Run(ref, -1.0, 9)
    nxt = 3 * E
    for x in (a, b):
        x.eng.reset(x.obs, offset=0)
    for k in range(4):
        for x in (a, b):
            x.steps(x.T)
        if k == 2:   # a refill of another window between the launch and the statistics
            for x in (a, b):
                x.eng.pool_refill(cfg, cfg.seed, nxt, ((k + 2) % 3) * E, E)
            nxt += E
        (sa, oa), (sb, ob) = a.stats_reset(((k + 1) % 3) * E), b.stats_reset(((k + 1) % 3) * E)
        _same(sa, sb, f"episode {k}: statistics")
        _same(oa, ob, f"episode {k}: reset observation")
        assert eng.last_stats_route == (0 if k == 2 else 1), (k, eng.last_stats_reason)
        if k == 2:
            assert "refilled" in eng.last_stats_reason
        for x in (a, b):
            x.eng.pool_refill(cfg, cfg.seed, nxt, ((k + 2) % 3) * E, E)
        nxt += E
    assert eng.pool_refill_overflows == 0
    eng.close(); ref.close()


def test_replayed_back_to_back_sessions(monkeypatch):
    """The reference fixtures whose next EV plugs in right behind its predecessor's departure, tiled to a batch and replayed over whole
    episodes: the in-launch statistics equal the kernel's whichever route the fixture's shape takes."""
    from conftest import B2B_FILES, load_golden
    from ev2gym_amd import _abi
    assert B2B_FILES
    for path in B2B_FILES:
        z, batch, rk, sk = load_golden(path)
        big = batch.tile(64)
        eng, ref = _engines(big, rk, sk, _abi.FLAG_LOG_SOC, monkeypatch)
        lo = 0.0 if sk == _abi.STATE_KINDS["PublicPST"] else -1.0
        a, b = _Run(eng, lo, 77), _Run(ref, lo, 77)
        for ep in range(2):
            for x in (a, b):
                x.eng.reset(x.obs, offset=0)
                x.steps(x.T)
            _same(a.stats(), b.stats(), f"{os.path.basename(path)} episode {ep}")
            wide_one = eng.last_launch_specialisation == 2 and eng.P > 32
            assert eng.last_stats_route == (1 if wide_one else 0), (path, eng.P, eng.last_launch_specialisation, eng.last_stats_reason)
        eng.close(); ref.close()
