"""CU balance (include/ev2g.h: ev2g_last_launch_balance; csrc/ev2g_balance_host.h): a fast-forwarding persistent launch from step 0 is handed a
permutation of the env groups, so that heavy and light groups share a CU.  Where a workgroup runs and which group it steps must not change a bit.

Every case compares a whole-episode persistent launch BIT FOR BIT with the same launch of an engine loaded with EV2G_NO_CU_BALANCE=1 and with
single-step launches: the last step's observation / reward / done / mask, the 17 statistics (which carry the episode accumulators and everything
derived from the SoC log) and ev2g_peek of every env (port and session state, history rows).  An env that no workgroup stepped, or that two did,
differs in all of them.  Every case asserts what the reporter says, so that a map that is silently never used fails.

The path needs one env per wavefront, i.e. 33 .. 64 ports: 33 is the smallest env that reaches it."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2G, RK0 = "V2G_profit_max_loads", "ProfitMax_TrPenalty_UserIncentives"


def _pool(M, P, seed=11, **kw):
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    return generate_native(GenConfig.v2g_profit_plus_loads(M, P, 1, seed=seed, **kw))


class _Run:
    def __init__(self, batch, E, acts_h, monkeypatch, off=False, flags=0, stream=None):
        from ev2gym_amd import _abi
        from ev2gym_amd.engine import Engine
        if off:
            monkeypatch.setenv("EV2G_NO_CU_BALANCE", "1")
        try:
            self.eng = eng = Engine(batch, _abi.REWARD_KINDS[RK0], _abi.STATE_KINDS[V2G], device=0, flags=_abi.FLAG_LOG_SOC | flags, n_active_envs=E,
                                    stream=stream)
        finally:
            if off:
                monkeypatch.delenv("EV2G_NO_CU_BALANCE")
        self.E, self.P, self.T = eng.E, eng.P, eng.T
        self.acts = eng.empty(acts_h.shape).upload(acts_h)
        self.obs, self.rew = eng.empty((eng.E, eng.D)), eng.empty((eng.E,))
        self.done, self.mask = eng.empty((eng.E,), np.uint8), eng.empty((eng.E, eng.P), np.uint8)

    def launch(self, k, persistent=True):
        eng, EP = self.eng, self.E * self.P
        t0 = eng.current_step
        if persistent:
            eng.step_n(k, self.acts.at(t0 * EP), EP, self.obs, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=True)
        else:
            for t in range(t0, t0 + k):
                eng.step_n(1, self.acts.at(t * EP), EP, self.obs, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=False)

    def results(self, stats=None):
        eng = self.eng
        eng.check_faults()
        r = dict(obs=self.obs.to_host(), reward=self.rew.to_host(), done=self.done.to_host(), mask=self.mask.to_host(),
                 stats=(eng.stats() if stats is None else stats.to_host()).copy())
        for e in range(eng.E):
            for key, v in eng.peek(e).items():
                r[f"env{e}.{key}"] = np.asarray(v).copy()
        return r


def _acts(T, E, P, seed=23):
    from ev2gym_amd.engine import host_uniform
    return host_uniform(T * E * P, seed, -1.0, 1.0).reshape(T, E, P)


def _same(got, exp, what):
    bad = [k for k in exp if np.ascontiguousarray(got[k]).tobytes() != np.ascontiguousarray(exp[k]).tobytes()]
    assert not bad, f"{what}: {bad[:8]} ({len(bad)} arrays differ)"


def _episode_three_ways(batch, E, monkeypatch, offset=0):
    """One whole episode on window `offset`: balanced persistent launch, the same with EV2G_NO_CU_BALANCE=1, single-step launches.  -> the reporter's
    answer for the balanced launch."""
    T, P = batch.n_steps, batch.n_ports
    acts_h = _acts(T, E, P)
    on, off = _Run(batch, E, acts_h, monkeypatch), _Run(batch, E, acts_h, monkeypatch, off=True)
    try:
        for r in (on, off):
            r.eng.reset(offset=offset)
            r.launch(T)
        said, said_off = on.eng.last_launch_balance, off.eng.last_launch_balance
        assert on.eng.last_launch_specialisation == 2 and on.eng.last_launch_fast_forwarded[0] >= 0
        assert said_off[0] is False and said_off[1] == 0 and "EV2G_NO_CU_BALANCE" in said_off[2], said_off
        r_on, r_off = on.results(), off.results()
        assert on.eng.last_stats_route == 1, on.eng.last_stats_reason   # (the balanced launch computed the statistics in its tail)
        off.eng.reset(offset=offset)
        off.launch(T, persistent=False)
        r_one = off.results()
        _same(r_on, r_off, f"E = {E}, P = {P}, offset {offset}: differs from the same launch with EV2G_NO_CU_BALANCE=1")
        _same(r_on, r_one, f"E = {E}, P = {P}, offset {offset}: differs from single-step launches")
        return said
    finally:
        on.eng.close(); off.eng.close()


def test_more_groups_than_the_chip_holds(monkeypatch):
    """E = 4100: 1025 groups, one more than 256 CUs hold at four each, no multiple of 8 (the kernel's own map is the identity there), and the last
    group is partial."""
    said = _episode_three_ways(_pool(4100, 33), 4100, monkeypatch)
    print("  balance:", said)
    assert said[0] and said[1] > 512 and said[2] == "", said   # (a sort by weight moves nearly every group)


def test_partial_group_fewer_groups_than_cus(monkeypatch):
    said = _episode_three_ways(_pool(37, 33), 37, monkeypatch)
    assert said[0] and 0 < said[1] <= 10 and said[2] == "", said


def test_bench_shape_1024_envs(monkeypatch):
    """50 ports, the benchmark's generator and order, one workgroup per CU."""
    said = _episode_three_ways(_pool(1024, 50, seed=0).sorted_by_busy_window(1024), 1024, monkeypatch)
    assert said[0] and said[1] > 128 and said[2] == "", said


def test_windows_of_a_pool_and_slot_reuse(monkeypatch):
    """Episodes on 70 different windows of one pool, moved on by stats_reset like the benchmark's loop: offsets k * E have their maps from the load,
    the odd ones are built at the window's first launch, and the 65th distinct window re-uses the oldest of the 64 slots; then a window seen before."""
    E, M = 8, 80
    batch = _pool(M, 33, seed=4)
    T, P = batch.n_steps, batch.n_ports
    acts_h = _acts(T, E, P)
    on, off = _Run(batch, E, acts_h, monkeypatch), _Run(batch, E, acts_h, monkeypatch, off=True)
    try:
        offsets = [0, 8, 3] + list(range(9, 75)) + [3, 0]
        st_on, st_off = on.eng.empty((E, 17)), off.eng.empty((E, 17))
        for r in (on, off):
            r.eng.reset(offset=offsets[0])
        for i, o in enumerate(offsets):
            nxt = offsets[(i + 1) % len(offsets)]
            on.launch(T); off.launch(T)
            said = on.eng.last_launch_balance
            assert said[0] and said[2] == "", (o, said)
            assert on.eng.scenario_offset == o
            on.eng.stats_reset(st_on, on.obs, offset=nxt); off.eng.stats_reset(st_off, off.obs, offset=nxt)
            a, b = st_on.to_host(), st_off.to_host()
            assert a.tobytes() == b.tobytes(), f"episode {i} on window {o}: statistics differ from EV2G_NO_CU_BALANCE=1"
            assert on.obs.to_host().tobytes() == off.obs.to_host().tobytes()
        on.launch(T); off.launch(T)
        _same(on.results(), off.results(), "after 71 episodes")
    finally:
        on.eng.close(); off.eng.close()


def test_launches_that_keep_the_kernels_own_map(monkeypatch):
    """A launch from step 3, a single step, an episode of 300 steps and a refillable handle: each keeps today's map and says why; results as ever."""
    from ev2gym_amd import _abi
    E, P = 12, 33
    batch = _pool(E, P, seed=6)
    T = batch.n_steps
    acts_h = _acts(T, E, P)
    on, off = _Run(batch, E, acts_h, monkeypatch), _Run(batch, E, acts_h, monkeypatch, off=True)
    try:
        for r in (on, off):
            r.eng.reset()
            r.launch(3)
        assert on.eng.last_launch_balance[0] is True
        for r in (on, off):
            r.launch(T - 4)
        said = on.eng.last_launch_balance
        assert said[0] is False and said[1] == 0 and "step 0" in said[2], said
        for r in (on, off):
            r.launch(1)
        said = on.eng.last_launch_balance
        assert said[0] is False and "fast-forward" in said[2], said
        _same(on.results(), off.results(), "launches 3 + (T - 4) + 1")
    finally:
        on.eng.close(); off.eng.close()
    long = _pool(8, 33, seed=6, simulation_length=300, timescale=5)
    r = _Run(long, 8, _acts(300, 8, 33), monkeypatch)
    try:
        r.eng.reset(); r.launch(300)
        said = r.eng.last_launch_balance
        assert said[0] is False and "256 steps" in said[2], said
        assert r.eng.last_launch_fast_forwarded[0] >= 0
    finally:
        r.eng.close()
    r = _Run(batch, E, acts_h, monkeypatch, flags=_abi.FLAG_REFILLABLE)
    try:
        r.eng.reset(); r.launch(T)
        said = r.eng.last_launch_balance
        assert said[0] is False and "REFILLABLE" in said[2], said
    finally:
        r.eng.close()


def test_two_handles_on_two_streams(monkeypatch):
    """Two handles step different windows at once on two streams: whoever shares a CU with whom, each gets what it gets alone."""
    import torch
    E, P = 2048, 33
    batch = _pool(2 * E, P, seed=8)
    T = batch.n_steps
    acts_h = _acts(T, E, P)
    s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    a, b = _Run(batch, E, acts_h, monkeypatch, stream=s1.cuda_stream), _Run(batch, E, acts_h, monkeypatch, stream=s2.cuda_stream)
    alone = _Run(batch, E, acts_h, monkeypatch, off=True)
    try:
        a.eng.reset(offset=0); b.eng.reset(offset=E)
        a.eng.synchronize(); b.eng.synchronize()
        a.launch(T); b.launch(T)   # (queued back to back on two streams: the launches overlap)
        assert a.eng.last_launch_balance[0] and b.eng.last_launch_balance[0]
        ra, rb = a.results(), b.results()
        for off_, got in ((0, ra), (E, rb)):
            alone.eng.reset(offset=off_); alone.launch(T)
            _same(got, alone.results(), f"window {off_} next to another handle's launch")
    finally:
        a.eng.close(); b.eng.close(); alone.eng.close()
