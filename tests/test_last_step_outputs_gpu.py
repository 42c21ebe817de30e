"""Stride-0 outputs of a persistent launch are written in the launch's LAST step only (include/ev2g.h: "stride 0 = one buffer that holds the
launch's last step").  After the launch the four output buffers -- every column of every row -- and all state must be, bit for bit, what a chain
of single-step launches leaves; on the fast path also what the last row of a launch that KEEPS every row (step strides) holds."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2G, PST = "V2G_profit_max_loads", "PublicPST"
# name, state, reward, envs, chargers, transformers, float32 hand-over, the specialisation the stride-0 launch must get, the one a strided launch gets (None: not run)
SHAPES = [
    ("cfg2_like", V2G, "ProfitMax_TrPenalty_UserIncentives", 9, 50, 1, False, 2, 3),      # head-table state, one env per wavefront (ragged last workgroup)
    ("cfg3_like", PST, "SquaredTrackingErrorReward", 10, 20, 1, False, 2, 3),             # PublicPST, three envs per wavefront (ragged last wavefront)
    ("narrow", V2G, "ProfitMax_TrPenalty_UserIncentives", 11, 12, 1, False, 1, 0),        # P < 15: the second head pair and the tail loop of the narrow kernel
    ("f32_handover", V2G, "ProfitMax_TrPenalty_UserIncentives", 9, 50, 1, True, 2, None),
    ("f32_narrow", V2G, "profit_maximization", 7, 12, 1, True, 1, None),
    ("big", V2G, "ProfitMax_TrPenalty_UserIncentives", 3, 520, 4, False, 5, None),        # ev2g_step_big
]


def _windows(batch, T, E):
    """Launch lengths k (last step t = k - 1, which ends at step number k) inside the episode: one whose last step finds an env with every port empty
    and nothing arriving (the fast path's empty-wavefront branch where an env owns a wavefront), one whose last step has an arrival and / or a departure."""
    st, ta, td = batch.arrays["env_session_start"], batch.arrays["ev_t_arr"], batch.arrays["ev_t_dep"]
    occ, arr, dep = np.zeros((E, T + 2), int), np.zeros((E, T + 2), int), np.zeros((E, T + 2), int)
    for e in range(E):
        for s in range(int(st[e]), int(st[e + 1])):
            a, d = int(ta[s]), int(td[s])
            if a > T:
                continue
            occ[e, max(a, 0):min(d, T) + 1] += 1
            arr[e, max(a, 0)] += 1
            if d <= T:
                dep[e, d] += 1
    ks = range(2, T)
    quiet = [k for k in ks if ((occ[:, k - 1] == 0) & (arr[:, k] == 0)).any()]
    both = [k for k in ks if arr[:, k].any() and dep[:, k - 1].any()]
    either = [k for k in ks if arr[:, k].any() or dep[:, k - 1].any()]
    some_empty = [k for k in ks if occ[:, k - 1].min() < batch.n_chargers]
    k_event = (both or either)[len(both or either) // 2]
    k_quiet = next((k for k in (quiet or some_empty) if k != k_event))
    return k_quiet, bool(quiet), k_event


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
        eng = self.eng
        eng.reset()
        self.obs.upload(np.full(self.obs.shape, np.nan, self.obs.dtype))
        self.rew.upload(np.full(self.rew.shape, np.nan))
        self.done.upload(np.full(self.done.shape, 0xAB, np.uint8))
        self.mask.upload(np.full(self.mask.shape, 0xAB, np.uint8))

    def launch(self, k, t0=0):
        """ONE persistent launch of k steps from step t0."""
        eng, EP = self.eng, self.eng.E * self.eng.P
        if self.f32:
            eng.set_extras(obs_f32=self.obs, actions_f32=self.acts.at(t0 * EP))
            eng.step_n(k, None, EP, None, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=True)
        else:
            eng.step_n(k, self.acts.at(t0 * EP), EP, self.obs, 0, self.rew, 0, self.done, 0, self.mask, 0, auto_reset=False, persistent=True)
        return eng.last_launch_specialisation

    def results(self):
        eng = self.eng
        eng.check_faults()
        out = dict(obs=self.obs.to_host(), reward=self.rew.to_host(), done=self.done.to_host(), mask=self.mask.to_host())
        state = {"stats": eng.stats().copy()}
        for e in range(eng.E):
            for key, v in eng.peek(e).items():
                state[f"env{e}.{key}"] = np.asarray(v).copy()
        return out, state


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_stride0_launch_leaves_the_last_steps_outputs_and_the_same_state(shape):
    """For k = T and two launch lengths that stop mid-episode (the last step over an empty env; the last step with an arrival / a departure):
    sentinel-filled outputs, one stride-0 persistent launch of k steps, against k single-step launches of a second handle (same scenarios, same
    actions) -- observation, reward, done, mask and the state (peek of every env: port state, histories, per-session results; the 17 statistics)
    bit for bit, no sentinel left anywhere -- and, where the shape has a fast-path instantiation, against the last row of a launch with step strides.

    The one tolerance: ev2g_step_big adds charged / discharged energy up per lane over the LAUNCH and reduces once (ev2g_step_big.h), so launches of
    different lengths group those two sums differently; `total_energy_charged` / `total_energy_discharged` of the big shape are held to 1e-12
    relative (the bound ev2g_step_big.h states and test_round6_gpu.py uses), everything else of that shape is exact too."""
    from ev2gym_amd.engine import host_uniform
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    name, state, reward, E, C, R, f32, want, want_strided = shape
    batch = generate_native(GenConfig.public_pst(E, C, seed=31) if state == PST else GenConfig.v2g_profit_plus_loads(E, C, R, seed=31))
    one, ref = None, None
    try:
        probe = _Run(batch, state, reward, f32, np.zeros(1))
        T, P, D = probe.eng.T, probe.eng.P, probe.eng.D
        probe.eng.close()
        acts_h = host_uniform(T * E * P, 17, 0.0 if state == PST else -1.0, 1.0).reshape(T, E, P)
        if f32:
            acts_h = acts_h.astype(np.float32)
        k_quiet, env_wide, k_event = _windows(batch, T, E)
        if name in ("cfg2_like", "narrow", "f32_handover", "f32_narrow"):
            assert env_wide, "no step with a wholly empty env in this scenario draw: the empty-wavefront branch would go untested"
        one, ref = _Run(batch, state, reward, f32, acts_h), _Run(batch, state, reward, f32, acts_h)
        for k in (T, k_quiet, k_event):
            one.start()
            assert one.launch(k) == want, (one.eng.kernel_name, one.eng.last_launch_specialisation)
            got, got_state = one.results()
            ref.start()
            for t in range(k):
                ref.launch(1, t)
            exp, exp_state = ref.results()
            print(f"{name}: k = {k} of T = {T}")
            for key in exp:
                left = (got[key] == 0xAB) if got[key].dtype == np.uint8 else np.isnan(got[key])
                assert not left.any(), f"{key}: a sentinel survived the launch (k = {k}; {left.sum()} elements)"
                assert _bits(got[key]) == _bits(exp[key]), f"{key} after a {k}-step launch differs from {k} single-step launches ({(got[key] != exp[key]).sum()} elements)"
            assert (got["done"] == (1 if k == T else 0)).all() and set(np.unique(got["mask"])) <= {0, 1}
            bad = []
            for key in exp_state:
                a, b = got_state[key], exp_state[key]
                if _bits(a) == _bits(b):
                    continue
                if want == 5 and key == "stats":   # (see the docstring)
                    loose = [2, 3]
                    tight = [c for c in range(a.shape[1]) if c not in loose]
                    err = np.abs(a[:, loose] - b[:, loose]) / np.maximum(1.0, np.abs(b[:, loose]))
                    print(f"  big: energy totals, max rel difference {err.max():.3e}")
                    if _bits(a[:, tight]) == _bits(b[:, tight]) and err.max() <= 1e-12:
                        continue
                bad.append(key)
            assert not bad, f"state after a {k}-step launch differs from {k} single-step launches: {bad}"
            if want_strided is not None:   # a launch that keeps every row: its last row is the stride-0 launch's one row
                eng = ref.eng
                o_k, r_k = eng.empty((k, E, D)), eng.empty((k, E))
                d_k, m_k = eng.empty((k, E), np.uint8), eng.empty((k, E, P), np.uint8)
                try:
                    eng.reset()
                    eng.step_n(k, ref.acts, E * P, o_k, E * D, r_k, E, d_k, E, m_k, E * P, auto_reset=False, persistent=True)
                    assert eng.last_launch_specialisation == want_strided
                    for key, buf in (("obs", o_k), ("reward", r_k), ("done", d_k), ("mask", m_k)):
                        assert _bits(buf.to_host()[k - 1]) == _bits(got[key]), f"{key}: the stride-0 row differs from the last row of the strided launch (k = {k})"
                finally:
                    for buf in (o_k, r_k, d_k, m_k):
                        buf.free()
    finally:
        for r in (one, ref):
            if r is not None:
                r.eng.close()
