"""The step loop of a persistent stride-0 launch is peeled (ev2g_step_wave.h): every step but the last runs a body without outputs -- the only one
that fast-forwards -- and the launch's last step a body with them.  Each case compares persistent launches BIT FOR BIT with the same steps as
single-step launches of a second handle: the last step's observation, reward, done and mask, the 17 statistics and ev2g_peek of every env (port and
session state, the history block).  The shapes are the smallest at which the peel can go wrong: k = 1 (the body with outputs alone), 2 and 3; launches
from step 0, from inside the episode, up to its end; a fast-forward pass that hands over directly to the peeled step; envs that never see an EV; a
partial group (5 envs: a workgroup with three wavefronts without an env); P = 33, 50, 64 (one env per wavefront), P = 20 PublicPST (three per
wavefront, no fast-forward) and the float32 hand-over.  Scenarios come from the benchmark's generator, a handful of envs each."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2G, PST = "V2G_profit_max_loads", "PublicPST"
RK0, RK1 = "ProfitMax_TrPenalty_UserIncentives", "SquaredTrackingErrorReward"


def _generated(E, P, state, seed=11):
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    return generate_native(GenConfig.public_pst(E, P, seed=seed) if state == PST else GenConfig.v2g_profit_plus_loads(E, P, 1, seed=seed))


def _with_sessions(g, sessions):
    """The generated batch `g` with its sessions replaced: per env a list of (charger, t_arr, t_dep); every other field of a session is taken from
    the generated ones in turn."""
    from ev2gym_amd import _abi
    from ev2gym_amd.scenario import ScenarioBatch
    E, a, S0 = g.n_envs, dict(g.arrays), g.n_sessions
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


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


class _Run:
    """One engine handle with sentinel-filled stride-0 output buffers."""

    def __init__(self, batch, state, reward, f32, acts_h):
        from ev2gym_amd import _abi
        from ev2gym_amd.engine import Engine
        self.eng = eng = Engine(batch, _abi.REWARD_KINDS[reward], _abi.STATE_KINDS[state], device=0, flags=_abi.FLAG_LOG_SOC)
        self.f32 = f32
        E, P, D = eng.E, eng.P, eng.D
        self.acts = eng.empty(acts_h.shape, np.float32 if f32 else np.float64).upload(acts_h)
        self.obs = eng.empty((E, D), np.float32 if f32 else np.float64)
        self.rew, self.done, self.mask = eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)

    def start(self):
        self.eng.reset()
        self.obs.upload(np.full(self.obs.shape, np.nan, self.obs.dtype))
        self.rew.upload(np.full(self.rew.shape, np.nan))
        self.done.upload(np.full(self.done.shape, 0xAB, np.uint8))
        self.mask.upload(np.full(self.mask.shape, 0xAB, np.uint8))

    def launch(self, k, persistent=False):
        """ONE launch of k steps from the handle's current step (the float32 hand-over exists as a persistent launch only)."""
        eng, EP = self.eng, self.eng.E * self.eng.P
        t0 = eng.current_step
        if self.f32:
            eng.set_extras(obs_f32=self.obs, actions_f32=self.acts.at(t0 * EP))
            eng.step_n(k, None, EP, None, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=True)
        else:
            eng.step_n(k, self.acts.at(t0 * EP), EP, self.obs, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=persistent)

    def results(self):
        eng = self.eng
        eng.check_faults()
        r = dict(obs=self.obs.to_host(), reward=self.rew.to_host(), done=self.done.to_host(), mask=self.mask.to_host(), stats=eng.stats().copy())
        for e in range(eng.E):
            for key, v in eng.peek(e).items():
                r[f"env{e}.{key}"] = np.asarray(v).copy()
        return r


def _check(batch, state, reward, windows, f32=False, want_spec=2, fast_forwarded=None):
    """`windows`: (t0, k) pairs -- t0 single-step launches from a reset, then ONE persistent launch of k steps -- each compared with t0 + k single-step
    launches of a second handle.  `fast_forwarded`: per window, what ev2g_last_launch_fast_forwarded must report for the persistent launch."""
    from ev2gym_amd.engine import host_uniform
    E, P, T = batch.n_envs, batch.n_ports, batch.n_steps
    acts_h = host_uniform(T * E * P, 29, 0.0 if state == PST else -1.0, 1.0).reshape(T, E, P)
    if f32:
        acts_h = acts_h.astype(np.float32)
    one, ref = _Run(batch, state, reward, f32, acts_h), _Run(batch, state, reward, f32, acts_h)
    try:
        assert one.eng.T == T
        for w, (t0, k) in enumerate(windows):
            assert t0 + k <= T
            one.start(); ref.start()
            for _ in range(t0):
                one.launch(1)
            one.launch(k, persistent=True)
            ff = one.eng.last_launch_fast_forwarded
            if k > 1:
                assert one.eng.last_launch_specialisation == want_spec, (one.eng.kernel_name, one.eng.last_launch_specialisation)
            for _ in range(t0 + k):
                ref.launch(1)
            got, exp = one.results(), ref.results()
            what = f"E = {E}, P = {P}, {state}{', float32 hand-over' if f32 else ''}: {t0} single steps, then one {k}-step launch (T = {T})"
            print(f"{what}: fast-forwarded {ff}")
            for key in ("obs", "reward", "done", "mask"):
                left = (got[key] == 0xAB) if got[key].dtype == np.uint8 else np.isnan(got[key])
                assert not left.any(), f"{what}: {key}: a sentinel survived ({left.sum()} elements)"
            assert (got["done"] == (1 if t0 + k == T else 0)).all()
            bad = [key for key in exp if _bits(got[key]) != _bits(exp[key])]
            assert not bad, f"{what}: differs from single-step launches in {bad}"
            if fast_forwarded is not None:
                assert ff == fast_forwarded[w], f"{what}: fast-forwarded {ff} (workgroup-steps, passes), built for {fast_forwarded[w]}"
    finally:
        one.eng.close(); ref.eng.close()


def _short_windows(T):
    """k = 1, 2, 3 from step 0, from inside the episode (ending before T) and up to T; the whole episode."""
    return [(0, 1), (0, 2), (0, 3), (37, 1), (37, 2), (38, 3), (T - 1, 1), (T - 2, 2), (T - 3, 3), (0, T)]


@pytest.mark.parametrize("P", [33, 50, 64])
def test_short_launches_one_env_per_wavefront(P):
    """Generated cfg2-like scenarios, 5 envs: the second workgroup holds one env and three wavefronts without one; P = 33 and 50 leave idle lanes."""
    batch = _generated(5, P, V2G)
    _check(batch, V2G, RK0, _short_windows(batch.n_steps))


def test_short_launches_three_envs_per_wavefront():
    """PublicPST with 20 ports: three envs per wavefront (7 envs: a ragged last wavefront), an instantiation without the fast-forward path."""
    batch = _generated(7, 20, PST)
    _check(batch, PST, RK1, _short_windows(batch.n_steps))


def test_float32_hand_over_two_steps():
    """The float32 hand-over instantiation (float32 actions in, the float32 observation out), k = 2: one step without outputs, one with."""
    batch = _generated(5, 50, V2G)
    T = batch.n_steps
    _check(batch, V2G, RK0, [(0, 2), (37, 2), (T - 2, 2)], f32=True)


def test_fast_forward_hands_over_to_the_peeled_step():
    """Every env's first EV arrives at the end of step 9: steps 0..8 are EV-free in both workgroups (5 envs: the second one has three wavefronts without
    an env).  A launch whose last step is step 9 (live), 8 or 5 (EV-free) goes from the fast-forward pass straight into the body with outputs."""
    sess = [[(e, 10, 60), (7 + e, 12, 40)] for e in range(5)]
    batch = _with_sessions(_generated(5, 50, V2G), sess)
    windows = [(0, 10), (0, 9), (3, 3), (0, 2), (4, 6), (0, 30)]
    want = [(2 * 9, 2), (2 * 8, 2), (2 * 2, 2), (2 * 1, 2), (2 * 5, 2), (2 * 9, 2)]
    _check(batch, V2G, RK0, windows, fast_forwarded=want)


def test_envs_that_never_see_an_ev():
    """No session starts inside the episode: every step of every launch but its last is fast-forwarded (at most 64 steps a pass), the last step runs the
    body with outputs over empty wavefronts; the whole-episode launch also computes the statistics in its tail."""
    g = _generated(5, 50, V2G)
    T = g.n_steps
    batch = _with_sessions(g, [[(e, T + 50, T + 80)] for e in range(5)])
    windows = [(0, T), (5, 3), (0, 2), (0, 1), (T - 70, 70)]
    want = [(2 * (T - 1), 2 * 2), (2 * 2, 2), (2 * 1, 2), (0, 0), (2 * 69, 2 * 2)]
    _check(batch, V2G, RK0, windows, fast_forwarded=want)
