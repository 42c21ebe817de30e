"""Launch stamps (include/ev2g.h: ev2g_last_step_n_kernel_ms, ev2g_last_launch_timing; csrc/ev2g_timing_host.h): a persistent ev2g_step_n that is one
launch of ev2g_step_wave's wide stride-0 instantiation (ev2g_last_launch_specialisation 2: the only one that carries the stamp sites, see
profiles/r28_launch_stamps.txt) is timed by the kernel's own readings of the constant-rate wall clock instead of a HIP-event pair around it.  The cases hold
that the stamps change nothing the launch computes (bit for bit against a handle loaded under EV2G_LAUNCH_TIMING=events), that a stamped reading is a
duration (positive, finite, not longer than the host's wall clock around the synchronised launch, the same when read twice), that the ring of the
last 32 timed calls behaves as it did with events alone, also with both kinds in it, and which kind each sort of call reports.

Shapes, from the library's generator -- the smallest that reach each instantiation:
  V2GProfitPlusLoads, 50 chargers, 5 envs: two workgroups, the second one partial, one env per wavefront, fast-forward and CU balance (the headline's)
  PublicPST, 20 chargers, 7 envs: three envs per wavefront, one partial workgroup (cfg3's)
  V2GProfitPlusLoads, 3 chargers, 9 envs: the narrow instantiation (specialisation 1: it keeps the event pair, and every case holds for it as such)"""
import math
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2G, PST = "V2G_profit_max_loads", "PublicPST"
RK0, RK1 = "ProfitMax_TrPenalty_UserIncentives", "SquaredTrackingErrorReward"
SHAPES = {"headline": (5, 50, V2G, RK0), "cfg3": (7, 20, PST, RK1), "narrow": (9, 3, V2G, RK0)}
STAMPED = {"headline": "stamps", "cfg3": "stamps", "narrow": "events"}   # what a persistent stride-0 launch of the shape reports
RING = 32


def _generated(E, P, state, pool=1, seed=11):
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    return generate_native(GenConfig.public_pst(pool * E, P, seed=seed) if state == PST else GenConfig.v2g_profit_plus_loads(pool * E, P, 1, seed=seed))


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


class _Run:
    """One engine handle on a stream of its own, the whole episode's actions and stride-0 output buffers."""

    def __init__(self, shape, events=False, pool=1, flags=0):
        from ev2gym_amd import _abi
        from ev2gym_amd.engine import Engine, host_uniform
        E, P, state, reward = SHAPES[shape]
        batch = _generated(E, P, state, pool)
        assert "EV2G_LAUNCH_TIMING" not in os.environ
        if events:
            os.environ["EV2G_LAUNCH_TIMING"] = "events"   # (read at load time)
        try:
            self.eng = eng = Engine(batch, _abi.REWARD_KINDS[reward], _abi.STATE_KINDS[state], device=0, flags=_abi.FLAG_LOG_SOC | flags, n_active_envs=E)
        finally:
            os.environ.pop("EV2G_LAUNCH_TIMING", None)
        assert eng.kernel_name.startswith("ev2g_step_wave") and (eng.E, eng.P) == (E, P)
        T, D = eng.T, eng.D
        self.E, self.P, self.T, self.EP = E, P, T, E * P
        self.acts = eng.empty((T, E, P)).upload(host_uniform(T * E * P, 29, 0.0 if state == PST else -1.0, 1.0).reshape(T, E, P))
        self.obs, self.rew, self.done, self.mask = eng.empty((E, D)), eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
        self.stats = eng.empty((E, _abi.N_STATS))
        self.offset = 0

    def launch(self, k=None, persistent=True, **kw):
        """ONE ev2g_step_n of k steps (default: up to the episode end) from the handle's current step."""
        eng = self.eng
        t0 = eng.current_step
        k = self.T - t0 if k is None else k
        args = dict(obs=self.obs, o_stride=0, reward=self.rew, r_stride=0, done=self.done, d_stride=0, mask=self.mask, m_stride=0)
        args.update(kw)
        eng.step_n(k, self.acts.at(t0 * self.EP), self.EP, auto_reset=False, persistent=persistent, **args)

    def episode_end(self, pool=1):
        self.offset = (self.offset + self.E) % (pool * self.E)
        self.eng.stats_reset(self.stats, self.obs, self.offset)

    def results(self):
        """The last step's outputs, ev2g_peek of every env, then the statistics through stats_reset."""
        eng = self.eng
        eng.check_faults()
        r = dict(obs=self.obs.to_host(), reward=self.rew.to_host(), done=self.done.to_host(), mask=self.mask.to_host())
        for e in range(eng.E):
            for key, v in eng.peek(e).items():
                r[f"env{e}.{key}"] = np.asarray(v).copy()
        self.episode_end()
        r["stats"] = self.stats.to_host()
        return r

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module", params=sorted(SHAPES))
def pair(request):
    """The same scenarios on a handle with stamps and on one loaded under EV2G_LAUNCH_TIMING=events."""
    a, b = _Run(request.param), _Run(request.param, events=True)
    yield request.param, a, b
    a.close(); b.close()


def test_stamps_change_nothing_the_launch_computes(pair):
    shape, st, ev = pair
    out = []
    for r in (st, ev):
        r.eng.reset()
        r.launch()
        out.append((r.eng.last_launch_timing, r.eng.last_step_n_kernel_ms(), r.eng.last_launch_specialisation, r.results()))
    (kind_s, ms_s, spec_s, got), (kind_e, ms_e, spec_e, exp) = out
    print(f"{shape}: stamps {ms_s * 1e3:.1f} us, events {ms_e * 1e3:.1f} us, specialisation {spec_s}")
    assert (kind_s, kind_e) == (STAMPED[shape], "events") and spec_s == spec_e == (2 if STAMPED[shape] == "stamps" else 1)
    assert ms_s > 0 and ms_e > 0
    assert (got["done"] == 1).all()
    bad = [key for key in exp if _bits(got[key]) != _bits(exp[key])]
    assert not bad, f"{shape}: a stamped launch differs from an event-timed one in {bad}"


def test_a_stamped_reading_is_a_duration(pair):
    shape, st, _ = pair
    eng = st.eng
    eng.reset()
    st.launch(); st.episode_end(); eng.synchronize()   # (warm: code objects loaded, the window's balance map built)
    eng.synchronize()
    t0 = time.perf_counter()
    st.launch()
    eng.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    ms, again = eng.last_step_n_kernel_ms(), eng.last_step_n_kernel_ms()
    print(f"{shape}: stamped {ms * 1e3:.1f} us inside {wall_ms * 1e3:.1f} us of wall clock")
    assert eng.last_launch_timing == STAMPED[shape]
    assert math.isfinite(ms) and 0 < ms <= wall_ms
    assert again == ms and eng.step_n_kernel_ms_back(0) == ms
    st.episode_end()


def test_the_ring_holds_the_last_32_launches(pair):
    shape, st, _ = pair
    eng = st.eng
    eng.reset()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(RING + 2):   # queued without a host synchronisation in between, across the episode ends
        st.launch()
        st.episode_end()
    eng.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    ms = [eng.step_n_kernel_ms_back(b) for b in range(RING)]
    print(f"{shape}: 32 readings {min(ms) * 1e3:.1f} .. {max(ms) * 1e3:.1f} us, sum {sum(ms):.3f} ms inside {wall_ms:.3f} ms")
    assert eng.last_launch_timing == STAMPED[shape]
    assert all(m > 0 for m in ms), ms
    assert eng.step_n_kernel_ms_back(RING) == -1.0
    assert sum(ms) <= wall_ms
    assert [eng.step_n_kernel_ms_back(b) for b in range(RING)] == ms
    eng.check_faults()


def test_both_kinds_in_one_ring(pair):
    shape, st, _ = pair
    eng = st.eng
    eng.reset()
    st.launch(3)
    a, kind_a = eng.step_n_kernel_ms_back(0), eng.last_launch_timing
    st.launch(2, persistent=False)
    b, kind_b = eng.step_n_kernel_ms_back(0), eng.last_launch_timing
    st.launch(3)
    c, kind_c = eng.step_n_kernel_ms_back(0), eng.last_launch_timing
    assert (kind_a, kind_b, kind_c) == (STAMPED[shape], "events", STAMPED[shape])
    assert min(a, b, c) > 0
    assert [eng.step_n_kernel_ms_back(i) for i in range(3)] == [c, b, a]   # each `back` reads its own call
    with pytest.raises(Exception, match="a step stride is negative or reaches 4 GiB"):
        st.launch(2, o_stride=-1)
    assert eng.step_n_kernel_ms_back(0) == -1.0 and eng.step_n_kernel_ms_back(1) == c and eng.last_launch_timing == ""
    assert eng.current_step == 8
    st.launch(2)   # the next call is readable again, the refused one stays behind it
    assert eng.step_n_kernel_ms_back(0) > 0 and eng.step_n_kernel_ms_back(1) == -1.0 and eng.step_n_kernel_ms_back(2) == c
    eng.step(st.acts.at(eng.current_step * st.EP), st.obs, st.rew, st.done, st.mask)   # a plain step: every reading is -1
    assert eng.step_n_kernel_ms_back(0) == -1.0 and eng.step_n_kernel_ms_back(2) == -1.0 and eng.last_launch_timing == ""
    eng.check_faults()


def test_which_kind_a_call_reports(pair):
    """A persistent call that is ONE launch of the wide stride-0 instantiation is stamped, from whatever step and however short; the instantiation for
    strided outputs, the narrow one and every call that queues several launches keep their event pair."""
    from ev2gym_amd import _abi
    shape, st, ev = pair
    eng, E, P, D = st.eng, st.E, st.P, st.eng.D

    def said(want):
        ms = eng.last_step_n_kernel_ms()
        assert (eng.last_launch_timing, ms > 0) == (want, True), (shape, want, eng.last_launch_timing, ms)

    eng.reset()
    for _ in range(3):
        eng.step(st.acts.at(eng.current_step * st.EP), st.obs, st.rew, st.done, st.mask)
    st.launch(5); said(STAMPED[shape])                  # from step 3: one launch
    st.launch(1); said(STAMPED[shape])                  # k = 1: one launch
    obs, rew = eng.empty((4, E, D)), eng.empty((4, E))
    done, mask = eng.empty((4, E), np.uint8), eng.empty((4, E, P), np.uint8)
    st.launch(4, obs=obs, o_stride=E * D, reward=rew, r_stride=E, done=done, d_stride=E, mask=mask, m_stride=E * P); said("events")   # strided outputs: one launch, of an instantiation without the stamp sites
    st.launch(4, persistent=False); said("events")      # the per-step chain
    ev.eng.reset()
    ev.launch(5)
    assert ev.eng.last_launch_timing == "events" and ev.eng.last_step_n_kernel_ms() > 0   # the switch
    eng.check_faults()
    # a refillable handle: its persistent launch is one launch of ev2g_step_wave like any other
    r = _Run(shape, flags=_abi.FLAG_REFILLABLE)
    try:
        r.eng.reset()
        r.launch()
        assert r.eng.last_launch_timing == STAMPED[shape] and r.eng.last_step_n_kernel_ms() > 0
        r.eng.check_faults()
    finally:
        r.close()


def test_two_handles_read_their_own_launches():
    """Two handles on two streams, launched alternately: a long launch (the whole episode) on one, a short one (2 steps) on the other."""
    a, b = _Run("headline"), _Run("headline")
    try:
        for r in (a, b):
            r.eng.reset()
            r.launch(); r.episode_end(); r.eng.synchronize()   # (warm)
        for _ in range(3):
            a.launch()
            b.launch(2)
            a.episode_end()
            b.launch(); b.episode_end()
        a.eng.synchronize(); b.eng.synchronize()
        long_a = [a.eng.step_n_kernel_ms_back(i) for i in range(3)]
        b_all = [b.eng.step_n_kernel_ms_back(i) for i in range(6)]   # newest first: rest, 2 steps, rest, 2 steps, ...
        short_b, rest_b = b_all[1::2], b_all[0::2]
        print(f"a: whole episodes {long_a}; b: 2 steps {short_b}, the rest {rest_b}")
        assert a.eng.last_launch_timing == "stamps" and b.eng.last_launch_timing == "stamps"
        assert min(long_a + b_all) > 0
        # T - 2 steps and T steps of the same scenarios take longer than 2 steps: a reading that was another handle's would break the order
        assert max(short_b) < min(rest_b) and max(short_b) < min(long_a)
        a.eng.check_faults(); b.eng.check_faults()
    finally:
        a.close(); b.close()
