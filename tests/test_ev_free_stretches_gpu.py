"""EV-free stretches of a persistent stride-0 launch are fast-forwarded (ev2g_step_wave's FFW path, include/ev2g.h:
ev2g_last_launch_fast_forwarded): a stretch of steps in which none of a workgroup's four envs holds an EV or receives one is done in one pass.

Every case runs a persistent stride-0 launch on hand-built scenarios and compares it BIT FOR BIT with (a) the same steps as single-step
launches and (b) the same launch of a second engine loaded with EV2G_NO_FAST_FORWARD=1: the history rows, the last step's observation /
reward / done / mask, the 17 statistics (which carry the episode accumulators and everything derived from the SoC log) and the port and
session state of every env (ev2g_peek).  The statistics are also held against the CPU oracle at the suite's 1e-9.  Every case asserts that
the reporter equals the count computed here in numpy from the sessions' windows -- a path that is silently never taken fails."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_MIN = 1   # EV2G_FF_N_MIN (ev2g_step_wave.h): the shortest stretch that is fast-forwarded
V2G, PST = "V2G_profit_max_loads", "PublicPST"
RK0, RK1, RK2, RK3 = "ProfitMax_TrPenalty_UserIncentives", "SquaredTrackingErrorReward", "profit_maximization", "SqTrError_TrPenalty_UserIncentives"
RTOL = 1e-9


def _batch(E, P, state, sessions, seed=5):
    """A generated batch of E envs x P single-port chargers whose sessions are replaced by `sessions`: per env a list of (charger, t_arr, t_dep);
    every other field of a session is taken from the generated ones in turn."""
    from ev2gym_amd.scenario import ScenarioBatch
    from ev2gym_amd import _abi
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    g = generate_native(GenConfig.public_pst(E, P, seed=seed) if state == PST else GenConfig.v2g_profit_plus_loads(E, P, 1, seed=seed))
    a = dict(g.arrays)
    S0 = g.n_sessions
    assert S0 > 0
    rows = [(e, cs, ta, td) for e in range(E) for (cs, ta, td) in sorted(sessions[e], key=lambda s: s[1])]
    idx = np.arange(len(rows)) % S0
    for n, _ in _abi.BATCH_ARRAYS:
        if n.startswith("ev_"):
            a[n] = g.arrays[n][idx].copy()
    a["ev_cs"] = np.array([r[1] for r in rows], np.int32)
    a["ev_t_arr"] = np.array([r[2] for r in rows], np.int32)
    a["ev_t_dep"] = np.array([r[3] for r in rows], np.int32)
    a["env_session_start"] = np.concatenate([[0], np.cumsum(np.bincount([r[0] for r in rows], minlength=E))]).astype(np.int64)
    return ScenarioBatch(E, g.n_steps, g.timescale, g.n_chargers, g.ports_per_charger, g.n_transformers, g.v2g_enabled, g.horizon, a).finalize()


def _group_free(batch):
    """[workgroups, T] bool: no env of the workgroup (four consecutive envs) holds an EV in step t or receives one at its end, i.e. no session
    with t_arr - 1 <= t <= t_dep.  Wavefronts without an env never constrain."""
    E, T = batch.n_envs, batch.n_steps
    st, ta, td = batch.arrays["env_session_start"], batch.arrays["ev_t_arr"], batch.arrays["ev_t_dep"]
    free = np.ones((-(-E // 4) * 4, T), bool)
    for e in range(E):
        for s in range(int(st[e]), int(st[e + 1])):
            free[e, max(int(ta[s]) - 1, 0):min(int(td[s]), T - 1) + 1] = False
    return free.reshape(-1, 4, T).all(axis=1)


def _expected(gfree, t0, k):
    """(workgroup-steps, passes) a launch of steps t0 .. t0 + k - 1 fast-forwards: at an EV-free step the workgroup skips to its next live step or
    to the launch's last step, whichever comes first and at most 64 steps at a time, when that is at least N_MIN steps away."""
    steps = stretches = 0
    for row in gfree:
        kk = 0
        while kk < k - 1:
            n = 0
            while n < 64 and kk + n < k - 1 and row[t0 + kk + n]:   # (one pass covers at most 64 steps, one per lane; a longer stretch takes another)
                n += 1
            if n >= max(N_MIN, 1):
                steps += n; stretches += 1; kk += n
            else:
                kk += 1
    return (steps, stretches) if k > 1 else (0, 0)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


class _Run:
    def __init__(self, batch, state, reward, acts_h, monkeypatch, off):
        from ev2gym_amd import _abi
        from ev2gym_amd.engine import Engine
        if off:
            monkeypatch.setenv("EV2G_NO_FAST_FORWARD", "1")
        try:
            self.eng = eng = Engine(batch, _abi.REWARD_KINDS[reward], _abi.STATE_KINDS[state], device=0, flags=_abi.FLAG_LOG_SOC)
        finally:
            if off:
                monkeypatch.delenv("EV2G_NO_FAST_FORWARD")
        E, P, D = eng.E, eng.P, eng.D
        self.acts = eng.empty(acts_h.shape).upload(acts_h)
        self.obs, self.rew = eng.empty((E, D)), eng.empty((E,))
        self.done, self.mask = eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)

    def start(self):
        self.eng.reset()
        self.obs.upload(np.full(self.obs.shape, np.nan))
        self.rew.upload(np.full(self.rew.shape, np.nan))
        self.done.upload(np.full(self.done.shape, 0xAB, np.uint8))
        self.mask.upload(np.full(self.mask.shape, 0xAB, np.uint8))

    def launch(self, k, persistent=True):
        eng, EP = self.eng, self.eng.E * self.eng.P
        t0 = eng.current_step
        if persistent:
            eng.step_n(k, self.acts.at(t0 * EP), EP, self.obs, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=True)
        else:
            for t in range(t0, t0 + k):
                eng.step_n(1, self.acts.at(t * EP), EP, self.obs, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=False)

    def results(self):
        eng = self.eng
        eng.check_faults()
        r = dict(obs=self.obs.to_host(), reward=self.rew.to_host(), done=self.done.to_host(), mask=self.mask.to_host(), stats=eng.stats().copy())
        for e in range(eng.E):
            for key, v in eng.peek(e).items():
                r[f"env{e}.{key}"] = np.asarray(v).copy()
        return r


def _same(got, exp, what):
    bad = [k for k in exp if _bits(got[k]) != _bits(exp[k])]
    assert not bad, f"{what}: {bad}"


def _oracle_stats(batch, state, reward, acts_h, n):
    from ev2gym_amd import _abi
    from oracle.oracle import Oracle
    ora = Oracle(batch, _abi.REWARD_KINDS[reward], _abi.STATE_KINDS[state])
    ora.reset()
    for t in range(n):
        ora.step(acts_h[t].copy())
    st = ora.stats().copy()
    ora.close()
    return st


def _close(a, b, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert (np.isnan(a) == np.isnan(b)).all(), f"{what}: NaN pattern differs"
    err = np.nan_to_num(np.abs(a - b) / np.maximum(1.0, np.abs(np.nan_to_num(b))))
    assert err.max(initial=0.0) <= RTOL, f"{what}: max rel err {err.max():.3e}"


def _check(batch, state, reward, launches, monkeypatch, eligible=True, want_spec=2, expect=None, oracle=True):
    """`launches`: a list of windows, each a list of (k, persistent) launched one after the other from a reset; the windows' persistent launches are
    compared with single-step launches and with the switched-off engine, their counts with the numpy rule."""
    from ev2gym_amd.engine import host_uniform
    E, P, T = batch.n_envs, batch.n_ports, batch.n_steps
    acts_h = host_uniform(T * E * P, 23, 0.0 if state == PST else -1.0, 1.0).reshape(T, E, P)
    gfree = _group_free(batch)
    on, off = _Run(batch, state, reward, acts_h, monkeypatch, False), _Run(batch, state, reward, acts_h, monkeypatch, True)
    try:
        for window in launches:
            on.start(); off.start()
            total = 0
            for k, persistent in window:
                t0 = on.eng.current_step
                on.launch(k, persistent); off.launch(k, persistent)
                got, none = on.eng.last_launch_fast_forwarded, off.eng.last_launch_fast_forwarded
                want = _expected(gfree, t0, k) if (eligible and persistent) else (0, 0)
                print(f"  launch t0 = {t0} k = {k} persistent = {persistent}: fast-forwarded {got}, numpy {want}")
                assert none == (0, 0), f"EV2G_NO_FAST_FORWARD=1 still fast-forwards: {none}"
                assert got == want, f"launch t0 = {t0}, k = {k}: fast-forwarded {got} (steps, stretches), the sessions' windows give {want}"
                if persistent and k > 1:
                    assert on.eng.last_launch_specialisation == want_spec, (on.eng.last_launch_specialisation, on.eng.last_launch_general_reason)
                total += want[0]
            if expect is not None:
                assert total == expect, f"this case was built to fast-forward {expect} workgroup-steps, the numpy rule gives {total}"
            n = on.eng.current_step
            r_on, r_off = on.results(), off.results()
            inl = eligible and want_spec == 2 and n == T and window[-1][1] and window[-1][0] > 1   # the launch that ended the episode computed its statistics in its tail
            if inl:
                assert on.eng.last_stats_route == 1, on.eng.last_stats_reason
            off.start()
            off.launch(n, persistent=False)
            r_one = off.results()
            if inl:
                assert off.eng.last_stats_route == 0   # (single-step launches: the statistics kernel)
            what = f"E = {E}, P = {P}, {reward}, launches {window}"
            _same(r_on, r_one, f"{what}: differs from single-step launches")
            _same(r_on, r_off, f"{what}: differs from the same launches with EV2G_NO_FAST_FORWARD=1")
            assert not np.isnan(r_on["obs"]).any() and not (r_on["mask"] == 0xAB).any()
            if oracle:
                _close(r_on["stats"], _oracle_stats(batch, state, reward, acts_h, n), f"{what}: statistics against the oracle")
    finally:
        on.eng.close(); off.eng.close()


T_ = 112


def _busy(first_arr=1):
    """Sessions that keep an env live from step first_arr - 1 to the episode's end."""
    return [(0, first_arr, 200)]


def test_no_session_in_a_workgroup(monkeypatch):
    """Envs 0..3 hold no session at all: the stretch is the whole launch but its last step (111 steps, two chunks of the pass); envs 4..7 are busy
    throughout (count 0 for that workgroup)."""
    batch = _batch(8, 50, V2G, [[]] * 4 + [_busy() + [(3, 5, 40), (7, 30, 111)]] * 4)
    _check(batch, V2G, RK0, [[(T_, True)]], monkeypatch, expect=T_ - 1)


@pytest.mark.parametrize("length", [N_MIN - 1, N_MIN, 2, 63, 64, 65])
def test_stretch_lengths(length, monkeypatch):
    """The first EV of the workgroup arrives at the end of step `length`: steps 0 .. length - 1 are one stretch."""
    sess = [[(1, length + 1, 100), (2, length + 4, 111)], [(0, length + 1, 90)], [(5, length + 9, 200)], [(4, length + 2, 105)]]
    batch = _batch(4, 50, V2G, sess)
    _check(batch, V2G, RK0, [[(length + 6, True)]], monkeypatch, expect=length if length >= N_MIN else 0)


@pytest.mark.parametrize("t_arr", [1, 2, 3])
def test_first_arrival_off_by_one(t_arr, monkeypatch):
    """t_arr = 1: step 0 is live (the EV arrives at its end); 2: one EV-free step; 3: two."""
    batch = _batch(4, 33, V2G, [[(0, t_arr, 60)], [(2, t_arr + 1, 50)], [(1, t_arr, 30), (1, 40, 70)], [(32, t_arr + 3, 80)]])
    _check(batch, V2G, RK0, [[(12, True)]], monkeypatch, expect=t_arr - 1)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_stretch_in_mid_episode(d, monkeypatch):
    """A departure in step 20 and the same port's next session arriving d steps later: back to back (d = 1) and d = 2 leave no EV-free step (the EV
    arrives at the END of step t_arr - 1), d = 3 leaves one."""
    sess = [[(6, 1, 20), (6, 20 + d, 60)]] * 4
    batch = _batch(4, 50, V2G, sess)
    _check(batch, V2G, RK0, [[(40, True)]], monkeypatch, expect=max(d - 2, 0))


def test_envs_that_wake_at_different_steps(monkeypatch):
    """Workgroup 0: four envs that wake at steps 30, 12, 50 and never -- the stretch ends at the earliest (step 11 is live: t_arr = 12 arrives at its
    end).  Workgroup 1: three envs EV-free for the whole episode and one never: nothing is fast-forwarded."""
    sess = [[(0, 31, 200)], [(9, 12, 200)], [(49, 51, 200)], [], [], [], [], _busy()]
    batch = _batch(8, 50, V2G, sess)
    _check(batch, V2G, RK0, [[(T_, True)]], monkeypatch, expect=11)


@pytest.mark.parametrize("E,P", [(5, 50), (9, 33)])
def test_wavefronts_without_an_env_and_idle_lanes(E, P, monkeypatch):
    """The last workgroup holds one env and three wavefronts without one; P = 33 / 50 leave idle lanes behind the env's last port."""
    sess = [[(e % P, 10 + e, 40 + e), (P - 1, 70, 90)] for e in range(E)]
    batch = _batch(E, P, V2G, sess)
    _check(batch, V2G, RK0, [[(T_, True)]], monkeypatch)


def test_launch_windows(monkeypatch):
    """Launches that start inside the episode (k = 2, 3 and k = T - t0), a stretch that runs past the launch's last step, two launches that split one
    stretch, and the episode-ending launch (in-launch statistics)."""
    sess = [[(0, 21, 60)], [(3, 25, 55)], [(7, 22, 58)], [(1, 30, 61)], [(2, 41, 80)]]   # workgroup 0: stretches 0..19 and 62..111; workgroup 1 (one env): 0..39 and 81..111
    batch = _batch(5, 50, V2G, sess)
    windows = [
        [(5, False), (2, True)], [(5, False), (3, True)], [(70, False), (T_ - 70, True)],
        [(10, True)],                                   # the stretch runs past the launch: 9 steps, not 10
        [(8, True), (30, True), (74, True)],            # one stretch split over two launches; the third ends the episode
    ]
    _check(batch, V2G, RK0, windows, monkeypatch)


@pytest.mark.parametrize("state,reward,P", [(V2G, RK0, 50), (V2G, RK1, 40), (V2G, RK2, 50)], ids=["RK0", "RK1", "RK2"])
def test_rewards_and_states(state, reward, P, monkeypatch):
    """The three compiled-in rewards; SquaredTrackingErrorReward reads the charge-power potential of the step before in a stretch's first step.
    (With a head-table state: the PublicPST instantiations do not carry the path, test_ineligible_shapes.)"""
    sess = [[(0, 6, 30), (1, 8, 33), (0, 50, 70)], [(2, 5, 31)], [(P - 1, 9, 28), (3, 52, 80)], [(4, 7, 35)]]
    batch = _batch(4, P, state, sess)
    _check(batch, state, reward, [[(T_, True)], [(3, False), (60, True)]], monkeypatch)


def test_ineligible_shapes(monkeypatch):
    """A reward selected at run time (general instantiation), three envs per wavefront (20-port PublicPST) and PublicPST with one env per wavefront (40
    ports: that state's instantiations are compiled without the path): nothing is fast-forwarded, results unchanged."""
    sess = [[(0, 20, 60)], [(3, 25, 55)], [(7, 22, 58)], [(1, 30, 61)]]
    _check(_batch(4, 50, V2G, sess), V2G, RK3, [[(T_, True)]], monkeypatch, eligible=False, want_spec=0)
    _check(_batch(6, 20, PST, sess + [[(5, 40, 90)], []]), PST, RK1, [[(T_, True)]], monkeypatch, eligible=False, want_spec=2)
    _check(_batch(4, 40, PST, sess), PST, RK1, [[(T_, True)]], monkeypatch, eligible=False, want_spec=2)


def test_generated_cfg2_pool(monkeypatch):
    """64 generated cfg2 scenarios, sorted by busy window like the benchmark's pool, one whole-episode launch."""
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    batch = generate_native(GenConfig.v2g_profit_plus_loads(64, 50, 1, seed=3)).sorted_by_busy_window(64)
    want = _expected(_group_free(batch), 0, batch.n_steps)
    assert want[0] > 16 * 20, "the generated pool has hardly any EV-free stretch: this case would test nothing"
    _check(batch, V2G, RK0, [[(batch.n_steps, True)]], monkeypatch)
