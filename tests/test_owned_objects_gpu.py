"""The device memory of the objects a handle owns (csrc/ev2g_host.hip: DevOwner's two pools, release_owned, owned_created, owned_check /
owned_destroy): ownership of wrappers, actor-critics and learners (tests/test_step_chain_gpu.py holds heuristics, links and grids), a close
with one live object of every kind, blocks that are zero at birth, a grid's state attached a second time and a policy's clipped block regrown
for a larger batch.

Shapes: the 34-bus grid context of tests/test_grid_state_gpu.py (5 envs x 33 one-port chargers, 8 steps, ev2g_step_v2<256>: the collector
steps through the registered float32 hand-over pair) and PublicPST, 4 and 8 envs x 20 ports, 12 steps.  Calls of 1 or 2 steps."""
import numpy as np
import pytest

from tests.test_grid_cpu import TOL
from tests.test_grid_gpu import run_batch
from tests.test_grid_state_gpu import WEIGHTS, Ctx
from tests.test_heuristics_gpu import PST_KINDS, _engine
from tests.test_onpolicy_gpu import Rows, _bits, _policy, _same_rows
from tests.test_step_chain_gpu import ARG, STALE, STATE, T_SHORT

pytestmark = pytest.mark.gpu

REPAIR = "Rescale_RepairLayer"
W = dict(base_weight=WEIGHTS[0], voltage_weight=WEIGHTS[1])


def _actor(eng, d_in):
    from ev2gym_amd.actor import init_mlp_weights
    return eng.mlp_create(*init_mlp_weights(d_in, eng.P, seed=9, h1=32, h2=32), out_lo=-1.0)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx(run_batch())
    yield c
    c.eng.close()


def test_wrappers_policies_and_learners_are_owned_and_close_frees_one_of_every_kind():
    from ev2gym_amd.engine import EngineError
    a, b = Ctx(run_batch()), Ctx(run_batch())
    eng, far = a.eng, b.eng
    E, P, D = eng.E, eng.P, eng.D
    assert P == eng.C   # (the repair layer's shape)
    x_obs, x_act = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
    eng.set_extras(obs_f32=x_obs, actions_f32=x_act)
    rows = Rows(eng, 1)
    idx = eng.empty((E,), np.int32).upload(np.arange(E, dtype=np.int32))
    wrap = eng.wrap_create(REPAIR)
    pol = _policy(eng, D, P, h=(32, 32), v=(32, 32))
    learner = eng.ppo_create(pol.ac, normalize_advantage=False)

    def alive():
        eng.reset_f32(rows.obs)   # (row 0 of the collector's block: the reset observation)
        rows.collect(pol, deterministic=True)
        eng.wrap_run(wrap, 1, a.d_act)
        eng.ppo_minibatch(learner, rows.obs, rows.act, rows.lp, rows.val, rows.val, idx, E)
        eng.ppo_sync(learner)
        eng.synchronize()
        assert eng.current_step == 2

    alive()
    for destroy, x in ((far.wrap_destroy, wrap), (far.ppo_destroy, learner), (far.ac_destroy, pol.ac)):
        destroy(x)   # not the owner: nothing happens
    alive()
    spare_w = eng.wrap_create(REPAIR)
    lone, bound = _policy(eng, D, P, h=(32, 32), v=(32, 32)), _policy(eng, D, P, h=(32, 32), v=(32, 32))
    lone_learner, bound_learner = eng.ppo_create(lone.ac), eng.a2c_create(bound.ac)
    for destroy, x in ((eng.wrap_destroy, spare_w), (eng.ppo_destroy, lone_learner), (eng.ac_destroy, bound.ac)):
        destroy(x)
        destroy(x)   # no longer in the handle's list: nothing happens
    eng.ac_seed(lone.ac, 1)   # (a policy outlives its learner)
    for call, what in ((lambda: eng.wrap_run(spare_w, 1, a.d_act), "ev2g_wrap_run: the wrapper"), (lambda: eng.ac_seed(bound.ac, 1), "ev2g_ac_seed: the actor-critic"),
                       (lambda: eng.ppo_sync(lone_learner), "ev2g_ppo_sync: the learner"),
                       (lambda: eng.ppo_sync(bound_learner), "ev2g_ppo_sync: the learner")):   # (it went with its policy)
        with pytest.raises(EngineError) as ei:
            call()
        assert ei.value.code == ARG and eng.last_error() == what + " was not created on this handle"
    alive()
    # one live object of every kind at the close: a link whose blocks of first use exist (under an agent: raw; under an actor: obs, obs32,
    # act32), the grid with its attached state, the policy that has collected
    agent, link, mlp = eng.heuristic_create("RoundRobin"), eng.link_create(0.3, 0.0, seed_act=5), _actor(eng, D)
    eng.reset()
    eng.link_run(link, 1, agent)
    eng.link_rollout(link, mlp, 1)
    eng.grid_observe(a.g)
    eng.grid_run(a.g, 1, agent, **W)
    assert eng.current_step == 3 and eng.grid_state_dim(a.g) == a.Dg
    eng.synchronize()
    eng.check_faults()
    eng.close(), far.close()   # with a heuristic, a link, a grid, a wrapper, two policies and a learner (and b's grid)


def test_a_grids_statistics_are_zero_at_birth(ctx):
    eng = ctx.eng
    g = eng.grid_create(ctx.net, (ctx.p_base, ctx.q_base), TOL, 100)
    stats = eng.grid_get_stats(g)   # before any step
    assert sorted(stats) == ["total_reward", "voltage_violation", "voltage_violation_counter", "voltage_violation_counter_per_step"]
    for name, x in stats.items():
        assert x.shape == (eng.E,) and not _bits(x).any(), name
    eng.grid_destroy(g)
    eng.synchronize()
    eng.check_faults()


def test_a_second_attach_replaces_the_state_and_gives_the_same_rollout(ctx):
    from ev2gym_amd.engine import EngineError
    eng, g = ctx.eng, ctx.g
    E, n_bus, k = eng.E, ctx.net.n_bus, 2
    mlp = _actor(eng, ctx.Dg)
    rew, vm = eng.empty((k, E)), eng.empty((k, E, n_bus))

    def rollout():
        eng.grid_rollout(g, mlp, k, reward=rew, r_stride=E, vm=vm, v_stride=E * n_bus, **W)
        eng.synchronize()
        return rew.to_host(), vm.to_host()

    def refused():
        with pytest.raises(EngineError) as ei:
            rollout()
        assert ei.value.code == STATE and eng.last_error() == "ev2g_grid_rollout: " + STALE % 0 and eng.current_step == 0

    eng.reset()
    eng.grid_observe(g)
    first = rollout()
    assert eng.current_step == k and np.abs(first[0]).max() > 0 and (first[1] > 0).all()
    eng.reset()
    assert eng.grid_state_attach(g, ctx.tf) == ctx.Dg == eng.grid_state_dim(g)
    refused()
    eng.grid_observe(g)
    assert eng.grid_state_attach(g, ctx.tf) == ctx.Dg   # (nothing has changed the envs' state: the attach alone drops the row)
    refused()
    eng.grid_observe(g)
    again = rollout()
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(first, again))
    assert eng.grid_state_dim(g) == ctx.Dg
    eng.mlp_destroy(mlp)
    eng.synchronize()
    eng.check_faults()


def test_a_policys_clipped_block_is_regrown_for_a_larger_batch():
    from ev2gym_amd.scenario_gen import GenConfig, generate
    four, eight = (generate(GenConfig.public_pst(E, 20, seed=31, spawn_multiplier=10, simulation_length=T_SHORT)) for E in (4, 8))
    eng, twin = _engine(four, PST_KINDS), _engine(eight, PST_KINDS)
    D, P, k = eng.D, eng.P, 2
    assert (eng.E, twin.E, twin.D, twin.P) == (4, 8, D, P)
    pol, fresh = _policy(eng, D, P, lo=0.0), _policy(twin, D, P, lo=0.0)   # (the same seed: the same weights)

    def collect(e, p):
        rows = Rows(e, k)
        e.reset_f32(rows.obs)
        rows.collect(p, deterministic=True)
        assert e.current_step == k
        return rows.host()

    small = collect(eng, pol)
    eng.load(eight)
    assert (eng.E, eng.D, eng.P) == (8, D, P)
    got, want = collect(eng, pol), collect(twin, fresh)
    assert got["act"].shape == (k, 8, P) and small["act"].shape == (k, 4, P)
    assert _same_rows(got, want)
    assert np.abs(got["act"]).max() > 0 and np.abs(got["obs"][k]).max() > 0
    for e in (eng, twin):
        e.synchronize()
        e.check_faults()
    pol.close(), fresh.close()
    eng.close(), twin.close()
