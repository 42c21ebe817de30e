"""What the entries that run k x (stages around a one-step launch) share on the host (csrc/ev2g_host.hip: timed_open / timed_close, run_chain,
chain_steps, owned_check / owned_destroy), beyond the values their own parity tests hold: the ring of timed calls, every refusal's code and
full message with the order in which the checks fire, and the ownership of heuristics, links and grids.

Shapes: PublicPST, 8 envs x 20 ports, and the default plugin pair, 8 envs x 30 ports on one transformer (both ev2g_step_wave), 12 steps; the
grid calls on the 34-bus context of tests/test_grid_state_gpu.py (5 envs x 33 ports, 8 steps, ev2g_step_v2<256>).  Calls of 2 or 3 steps.

A refused call leaves the ring in one of three states (read off the code of each entry, the same before and after run_chain existed):
  kept     refused before the slot was taken: both readings as they were                              (every argument / state check)
  invalid  refused after: step_n_kernel_ms_back(0) == -1, the earlier reading moved to back = 1        (ev2g_step_n: a stride the fast-path
           launch refuses)
  closed   the steps up to the episode end ran and ARE a timed call; the call still returns EV2G_ERR_DONE  (ev2g_step_n / ev2g_rollout with
           auto_reset off: they meet the end inside their loop, the step counter stops at T; every other entry refuses such a segment
           up front)"""
import numpy as np
import pytest

from tests.test_grid_cpu import TOL
from tests.test_grid_state_gpu import WEIGHTS, Ctx
from tests.test_grid_gpu import run_batch
from tests.test_heuristics_gpu import DEFAULT_KINDS, PST_KINDS, _engine

pytestmark = pytest.mark.gpu

ARG, STATE, DONE = -1, -3, -4
K = 2
T_SHORT = 12


class Box:
    """An engine with an agent, a link, an actor and the float32 hand-over pair registered, its blocks, and a second engine on the same
    scenarios whose objects are foreign to the first."""

    def __init__(self, kind):
        from ev2gym_amd.actor import init_mlp_weights
        from ev2gym_amd.scenario_gen import GenConfig, generate
        pst = kind == "pst"
        batch = generate(GenConfig.public_pst(8, 20, seed=31, spawn_multiplier=10, simulation_length=T_SHORT) if pst else
                         GenConfig.v2g_profit_plus_loads(8, 30, 1, seed=32, simulation_length=T_SHORT))
        kinds = PST_KINDS if pst else DEFAULT_KINDS
        self.eng, self.other = eng, other = _engine(batch, kinds), _engine(batch, kinds)
        assert eng.kernel_name.startswith("ev2g_step_wave") and (eng.E, eng.P, eng.T) == (8, 20 if pst else 30, T_SHORT)
        E, P, D, T = eng.E, eng.P, eng.D, eng.T
        self.EP = E * P
        self.acts = eng.empty((T, E, P))
        eng.fill_uniform(self.acts, T * E * P, 3, 0.0 if pst else -1.0, 1.0)
        self.obs, self.rew, self.done, self.mask = eng.empty((4, E, D)), eng.empty((4, E)), eng.empty((4, E), np.uint8), eng.empty((4, E, P), np.uint8)
        self.o32, self.a32 = eng.empty((5, E, D), np.float32), eng.empty((4, E, P), np.float32)
        self.x_obs, self.x_act = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
        self.register()
        self.agent, self.far_agent = eng.heuristic_create("RoundRobin"), other.heuristic_create("RoundRobin")
        p_delay = 0.3 if pst else 0.0   # (delayed observations are PublicPST's)
        self.link, self.far_link = eng.link_create(0.3, p_delay, seed_act=5, seed_obs=6), other.link_create(0.3, p_delay, seed_act=5, seed_obs=6)
        self.l32 = eng.link_obs_f32(self.link)
        lo = 0.0 if pst else -1.0
        self.mlp = eng.mlp_create(*init_mlp_weights(D, P, seed=9, h1=32, h2=32), out_lo=lo)
        self.wrong = eng.mlp_create(*init_mlp_weights(D, P + 1, seed=9, h1=32, h2=32), out_lo=lo)
        self.warm = heuristic_run

    def register(self):
        self.eng.set_extras(obs_f32=self.x_obs, actions_f32=self.x_act)

    def out(self, **kw):
        return {**dict(obs=self.obs, reward=self.rew, done=self.done, mask=self.mask), **kw}

    def prime(self, t=0):
        """Step counter t of a fresh episode; every float32 row an actor may read holds that counter's observation."""
        eng = self.eng
        eng.reset()
        if t:
            eng.step_n(t, self.acts, self.EP, persistent=True, auto_reset=0, **self.out())
        row = self.x_obs.to_host()   # (the registered pair's row is written by the reset and by every step)
        for dst in (self.l32, self.o32.ptr):   # the link's row, and row 0 of collect's block
            eng._check(eng._lib.ev2g_memcpy_h2d(eng._h, dst, row.ctypes.data, row.nbytes))

    def close(self):
        self.eng.close(), self.other.close()


class GBox:
    """The grid context, an actor on its state rows, a solver-only grid, a grid without an attached state, and a foreign context."""

    def __init__(self):
        from ev2gym_amd.actor import init_mlp_weights
        self.ctx, self.far = Ctx(run_batch()), Ctx(run_batch())
        self.eng, self.g, self.acts, self.far_g = self.ctx.eng, self.ctx.g, self.ctx.d_act, self.far.g
        eng = self.eng
        self.EP = eng.E * eng.P
        self.far_agent = self.far.eng.heuristic_create("RoundRobin")
        self.solver = eng.grid_create(self.ctx.net, None, TOL, 100)
        self.stateless = eng.grid_create(self.ctx.net, (self.ctx.p_base, self.ctx.q_base), TOL, 100)
        self.mlp = eng.mlp_create(*init_mlp_weights(self.ctx.Dg, eng.P, seed=9, h1=32, h2=32), out_lo=-1.0)
        self.wrong = eng.mlp_create(*init_mlp_weights(self.ctx.Dg + 1, eng.P, seed=9, h1=32, h2=32), out_lo=-1.0)
        self.w = dict(base_weight=WEIGHTS[0], voltage_weight=WEIGHTS[1])
        self.warm = grid_run

    def prime(self, t=0, observe=True):
        self.eng.reset()
        if t:
            self.eng.grid_run(self.g, t, None, self.acts, self.EP, **self.w)
        if observe:
            self.eng.grid_observe(self.g)

    def close(self):
        self.eng.close(), self.far.eng.close()


@pytest.fixture(scope="module", params=["pst", "default"])
def box(request):
    b = Box(request.param)
    yield b
    b.close()


@pytest.fixture(scope="module")
def gbox():
    b = GBox()
    yield b
    b.close()


# ---- the entries: call(b, k, **overrides) ----
def step_n(persistent):
    def call(b, k=K, **kw):
        b.eng.step_n(k, **{**b.out(actions=b.acts, a_stride=b.EP, auto_reset=0, persistent=persistent), **kw})
    return call


def rollout(b, k=K, m=None, **kw):
    b.eng.rollout(m or b.mlp, k, **{**dict(reward=b.rew, done=b.done, mask=b.mask), **kw})


def collect(b, k=K, m=None, **kw):
    b.eng.collect(m or b.mlp, k, **{**dict(obs=b.o32, actions=b.a32, reward=b.rew, done=b.done, mask=b.mask), **kw})


def heuristic_run(b, k=K, a="own", **kw):
    b.eng.heuristic_run(b.agent if a == "own" else a, k, **{**b.out(), **kw})


def link_run(b, k=K, l=None, a="own", **kw):
    b.eng.link_run(l or b.link, k, b.agent if a == "own" else a, **{**b.out(), **kw})


def link_rollout(b, k=K, l=None, m=None, **kw):
    b.eng.link_rollout(l or b.link, m or b.mlp, k, **{**dict(reward=b.rew, done=b.done, mask=b.mask), **kw})


def grid_run(b, k=K, g=None, a=None, **kw):
    b.eng.grid_run(g or b.g, k, a, **{**dict(actions=b.acts, a_stride=b.EP), **b.w, **kw})


def grid_run_observed(b, k=K, g=None, a=None, **kw):
    b.eng.grid_run_observed(g or b.g, k, a, **{**dict(actions=b.acts, a_stride=b.EP), **b.w, **kw})


def grid_rollout(b, k=K, g=None, m=None, **kw):
    b.eng.grid_rollout(g or b.g, m or b.mlp, k, **{**b.w, **kw})


BOX_ENTRIES = dict(step_n_per_step=step_n(False), step_n_persistent=step_n(True), rollout=rollout, collect=collect, heuristic_run=heuristic_run,
                   link_run=link_run, link_rollout=link_rollout)
GRID_ENTRIES = dict(grid_run=grid_run, grid_run_observed=grid_run_observed, grid_rollout=grid_rollout)


def _ring(eng):
    return eng.step_n_kernel_ms_back(0), eng.step_n_kernel_ms_back(1)


def _timed_twice(b, call):
    """Two successful calls in a row: each advances the counter by K and is the newest reading; the one before it moves to back = 1."""
    eng = b.eng
    b.prime()
    call(b)
    first, _ = _ring(eng)
    assert first > 0 and eng.current_step == K
    call(b)
    second, moved = _ring(eng)
    assert second > 0 and moved == first and eng.current_step == 2 * K
    eng.check_faults()


@pytest.mark.parametrize("name", sorted(BOX_ENTRIES))
def test_a_successful_call_takes_the_next_slot_of_the_ring(box, name):
    _timed_twice(box, BOX_ENTRIES[name])


@pytest.mark.parametrize("name", sorted(GRID_ENTRIES))
def test_a_successful_grid_call_takes_the_next_slot_of_the_ring(gbox, name):
    _timed_twice(gbox, GRID_ENTRIES[name])


def test_a_single_step_makes_the_reading_minus_one(box):
    box.prime()
    heuristic_run(box)
    assert box.eng.step_n_kernel_ms_back(0) > 0
    box.eng.step(box.acts, box.obs, box.rew, box.done, box.mask)
    assert box.eng.step_n_kernel_ms_back(0) == -1.0 and box.eng.step_n_kernel_ms_back(1) == -1.0
    heuristic_run(box)   # the next timed call is readable again
    assert box.eng.step_n_kernel_ms_back(0) > 0


# ---- refusals: (entry, what, step counter before, overrides, code, message behind "<entry>: ", ring, step counter after or None: unchanged) ----
LAST = "last"   # the episode's last step: a call of 3 steps would pass the end
END = "the segment would run past the episode end"
STOPPED = "episode finished before k_steps (auto_reset off)"
NEG = "negative step count or stride"
FAST = "a step stride is negative or reaches 4 GiB (unsupported by the fast-path kernel)"
NO_ACTOR_ROW = "register float32 observation (step stride 0) and action buffers with ev2g_set_step_extras first"
BOX_REFUSALS = [
    ("step_n_per_step", "count", 0, dict(k=-1), ARG, "bad arguments", "kept", None),
    ("step_n_per_step", "no actions", 0, dict(actions=None, unregister=True), ARG, "bad arguments", "kept", None),
    ("step_n_per_step", "end", LAST, dict(k=3), DONE, STOPPED, "closed", T_SHORT),
    ("step_n_per_step", "at the end", T_SHORT, dict(k=1), DONE, STOPPED, "closed", None),
    ("step_n_per_step", "stride", 0, dict(k=1, a_stride=1 << 29), ARG, FAST, "invalid", None),
    ("step_n_per_step", "count before stride", 0, dict(k=-1, a_stride=1 << 29), ARG, "bad arguments", "kept", None),
    ("step_n_persistent", "count", 0, dict(k=-1), ARG, "bad arguments", "kept", None),
    ("step_n_persistent", "end", LAST, dict(k=3), DONE, STOPPED, "closed", T_SHORT),
    ("step_n_persistent", "stride", 0, dict(o_stride=-1), ARG, FAST, "invalid", None),
    ("step_n_persistent", "stride before end", LAST, dict(k=3, o_stride=-1), ARG, FAST, "invalid", None),
    ("rollout", "count", 0, dict(k=-1), ARG, "bad arguments", "kept", None),
    ("rollout", "no float32 pair", 0, dict(unregister=True), ARG, NO_ACTOR_ROW, "kept", None),
    ("rollout", "actor", 0, dict(m="wrong"), ARG, "actor shape != (obs dim, ports)", "kept", None),
    ("rollout", "float32 pair before actor", 0, dict(m="wrong", unregister=True), ARG, NO_ACTOR_ROW, "kept", None),
    ("rollout", "end", LAST, dict(k=3), DONE, STOPPED, "closed", T_SHORT),
    ("collect", "null array", 0, dict(mask=None), ARG, "null argument (every transition array is required)", "kept", None),
    ("collect", "actor", 0, dict(m="wrong"), ARG, "actor shape != (obs dim, ports)", "kept", None),
    ("collect", "end", LAST, dict(k=3), DONE, END, "kept", None),
    ("collect", "actor before end", LAST, dict(k=3, m="wrong"), ARG, "actor shape != (obs dim, ports)", "kept", None),
    ("heuristic_run", "no agent", 0, dict(a=None), ARG, "null argument", "kept", None),
    ("heuristic_run", "foreign agent", 0, dict(a="far_agent"), ARG, "the heuristic was not created on this handle", "kept", None),
    ("heuristic_run", "stride", 0, dict(o_stride=-1), ARG, NEG, "kept", None),
    ("heuristic_run", "count", 0, dict(k=-1), ARG, NEG, "kept", None),
    ("heuristic_run", "end", LAST, dict(k=3), DONE, END, "kept", None),
    ("heuristic_run", "stride before end", LAST, dict(k=3, m_stride=-1), ARG, NEG, "kept", None),
    ("heuristic_run", "agent before stride", 0, dict(a="far_agent", a_stride=-1), ARG, "the heuristic was not created on this handle", "kept", None),
    ("heuristic_run", "stride of a block that is not passed", 0, dict(a_stride=-1), ARG, NEG, "kept", None),
    ("link_run", "foreign link", 0, dict(l="far_link"), ARG, "the link was not created on this handle", "kept", None),
    ("link_run", "foreign agent", 0, dict(a="far_agent"), ARG, "the heuristic was not created on this handle", "kept", None),
    ("link_run", "link before agent", 0, dict(l="far_link", a="far_agent"), ARG, "the link was not created on this handle", "kept", None),
    ("link_run", "stride", 0, dict(r_stride=-1), ARG, NEG, "kept", None),
    ("link_run", "no agent, no actions", 0, dict(a=None), ARG, "without an agent the raw actions are read from `actions`", "kept", None),
    ("link_run", "stride before actions", 0, dict(a=None, d_stride=-1), ARG, NEG, "kept", None),
    ("link_run", "end", LAST, dict(k=3), DONE, END, "kept", None),
    ("link_run", "actions before end", LAST, dict(k=3, a=None), ARG, "without an agent the raw actions are read from `actions`", "kept", None),
    ("link_rollout", "foreign link", 0, dict(l="far_link"), ARG, "the link was not created on this handle", "kept", None),
    ("link_rollout", "stride", 0, dict(r_stride=-1), ARG, "bad arguments", "kept", None),
    ("link_rollout", "actor", 0, dict(m="wrong"), ARG, "actor shape != (obs dim, ports)", "kept", None),
    ("link_rollout", "end", LAST, dict(k=3), DONE, END, "kept", None),
    ("link_rollout", "actor before end", LAST, dict(k=3, m="wrong"), ARG, "actor shape != (obs dim, ports)", "kept", None),
]
NO_STATE = "no state attached to the grid (ev2g_grid_state_attach)"
SOLVER = "the grid was created without base profiles (a solver only)"
STALE = "the grid's float32 row does not hold the state of step counter %d (ev2g_grid_observe first; a reset or a step outside the grid's calls invalidates it)"
GRID_REFUSALS = [
    ("grid_run", "foreign grid", 0, dict(g="far_g"), ARG, "the grid was not created on this handle", "kept", None),
    ("grid_run", "solver only", 0, dict(g="solver"), ARG, SOLVER, "kept", None),
    ("grid_run", "foreign agent", 0, dict(a="far_agent"), ARG, "the heuristic was not created on this handle", "kept", None),
    ("grid_run", "grid before agent", 0, dict(g="far_g", a="far_agent"), ARG, "the grid was not created on this handle", "kept", None),
    ("grid_run", "stride", 0, dict(v_stride=-1), ARG, NEG, "kept", None),
    ("grid_run", "solver only before stride", 0, dict(g="solver", v_stride=-1), ARG, SOLVER, "kept", None),
    ("grid_run", "no agent, no actions", 0, dict(actions=None), ARG, "without an agent the actions are read from `actions`", "kept", None),
    ("grid_run", "end", LAST, dict(k=3), DONE, END, "kept", None),
    ("grid_run", "actions before end", LAST, dict(k=3, actions=None), ARG, "without an agent the actions are read from `actions`", "kept", None),
    ("grid_run_observed", "no state", 0, dict(g="stateless"), STATE, NO_STATE, "kept", None),
    ("grid_run_observed", "solver only", 0, dict(g="solver"), ARG, SOLVER, "kept", None),
    ("grid_run_observed", "stride", 0, dict(go32_stride=-1), ARG, NEG, "kept", None),
    ("grid_run_observed", "no state before stride", 0, dict(g="stateless", go_stride=-1), STATE, NO_STATE, "kept", None),
    ("grid_run_observed", "foreign grid", 0, dict(g="far_g"), ARG, "the grid was not created on this handle", "kept", None),
    ("grid_run_observed", "foreign agent", 0, dict(a="far_agent"), ARG, "the heuristic was not created on this handle", "kept", None),
    ("grid_run_observed", "grid before agent", 0, dict(g="far_g", a="far_agent"), ARG, "the grid was not created on this handle", "kept", None),
    ("grid_run_observed", "no agent, no actions", 0, dict(actions=None), ARG, "without an agent the actions are read from `actions`", "kept", None),
    ("grid_run_observed", "actions before end", LAST, dict(k=3, actions=None), ARG, "without an agent the actions are read from `actions`", "kept", None),
    ("grid_run_observed", "end", LAST, dict(k=3), DONE, END, "kept", None),
    ("grid_run_observed", "stride before end", LAST, dict(k=3, m_stride=-1), ARG, NEG, "kept", None),
    ("grid_rollout", "foreign grid", 0, dict(g="far_g"), ARG, "the grid was not created on this handle", "kept", None),
    ("grid_rollout", "no state", 0, dict(g="stateless"), STATE, NO_STATE, "kept", None),
    ("grid_rollout", "solver only", 0, dict(g="solver"), ARG, SOLVER, "kept", None),
    ("grid_rollout", "stride", 0, dict(v_stride=-1), ARG, "bad arguments", "kept", None),
    ("grid_rollout", "actor", 0, dict(m="wrong"), ARG, "actor shape != (grid state dim, ports)", "kept", None),
    ("grid_rollout", "no observe", 0, dict(observe=False), STATE, STALE % 0, "kept", None),
    ("grid_rollout", "a step outside the grid's calls", 0, dict(outside=True), STATE, STALE % 1, "kept", None),
    ("grid_rollout", "end", LAST, dict(k=3), DONE, END, "kept", None),
    ("grid_rollout", "end before no observe", LAST, dict(k=3, observe=False), DONE, END, "kept", None),
    ("grid_rollout", "actor before end", LAST, dict(k=3, m="wrong"), ARG, "actor shape != (grid state dim, ports)", "kept", None),
]


def _refused(b, entries, row):
    from ev2gym_amd.engine import EngineError
    name, _, at, kw, code, msg, ring, after = row
    kw = {k: (getattr(b, v) if isinstance(v, str) else v) for k, v in kw.items()}
    eng = b.eng
    at = eng.T - 1 if at == LAST else at
    # two timed calls first: the ring has two readings to keep or to move
    b.prime()
    b.warm(b, 1)
    b.warm(b, 1)
    observe = kw.pop("observe", True)
    b.prime(at, observe) if isinstance(b, GBox) else b.prime(at)
    if kw.pop("outside", False):
        eng.step_n(1, b.acts, b.EP, auto_reset=0)
    if kw.pop("unregister", False):
        eng.set_extras()
    before, t0 = _ring(eng), eng.current_step
    assert before[0] > 0
    try:
        with pytest.raises(EngineError) as ei:
            entries[name](b, **kw)
    finally:
        if isinstance(b, Box):
            b.register()
    entry = "ev2g_step_n" if name.startswith("step_n") else "ev2g_" + name
    assert (ei.value.code, eng.last_error()) == (code, f"{entry}: {msg}")
    assert eng.current_step == (t0 if after is None else after)
    now = _ring(eng)
    if ring == "kept":
        assert now == before
    elif ring == "invalid":
        assert now == (-1.0, before[0])
    else:
        assert now[0] >= 0.0 and now[1] == before[0]
    eng.synchronize()
    eng.check_faults()


def _id(row):
    return f"{row[0]}-{row[1]}".replace(" ", "_")


@pytest.mark.parametrize("row", BOX_REFUSALS, ids=_id)
def test_refusals_keep_their_code_message_order_and_ring_state(box, row):
    _refused(box, BOX_ENTRIES, row)


@pytest.mark.parametrize("row", GRID_REFUSALS, ids=_id)
def test_grid_refusals_keep_their_code_message_order_and_ring_state(gbox, row):
    _refused(gbox, GRID_ENTRIES, row)


# ---- ownership ----
def test_destroy_twice_or_through_another_handle_is_a_no_op_and_close_frees_the_rest():
    from ev2gym_amd.engine import EngineError
    a, b = Ctx(run_batch()), Ctx(run_batch())
    eng, far = a.eng, b.eng
    E, P = eng.E, eng.P
    agent, link = eng.heuristic_create("ChargeAsLateAsPossible"), eng.link_create(0.3, 0.0, seed_act=5)
    w = dict(base_weight=WEIGHTS[0], voltage_weight=WEIGHTS[1])

    def alive():
        eng.reset()
        eng.heuristic_run(agent, 1)
        eng.link_run(link, 1, agent)
        eng.grid_run(a.g, 1, agent, **w)
        eng.synchronize()

    alive()
    for destroy, x in ((far.heuristic_destroy, agent), (far.link_destroy, link), (far.grid_destroy, a.g)):
        destroy(x)   # not the owner: nothing happens
    alive()
    spare = eng.heuristic_create("RoundRobin"), eng.link_create(0.0, 0.0), eng.grid_create(a.net, None, TOL, 100)
    for destroy, x, what in ((eng.heuristic_destroy, spare[0], "heuristic"), (eng.link_destroy, spare[1], "link"), (eng.grid_destroy, spare[2], "grid")):
        destroy(x)
        destroy(x)   # no longer in the handle's list: nothing happens
    for call, what in ((lambda: eng.heuristic_run(spare[0], 1), "ev2g_heuristic_run: the heuristic"), (lambda: eng.link_run(spare[1], 1, agent), "ev2g_link_run: the link"),
                       (lambda: eng.grid_solve(spare[2], a.d_act, a.d_act, 0), "ev2g_grid_solve: the grid")):
        with pytest.raises(EngineError) as ei:
            call()
        assert ei.value.code == ARG and eng.last_error() == what + " was not created on this handle"
    alive()
    eng.check_faults()
    eng.close(), far.close()   # with a live heuristic, link and grid (and b's grid) each
