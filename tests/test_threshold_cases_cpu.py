"""The threshold policies do what tests/threshold_cases.py says, measured on the CPU: the reference fixtures edge_*.npz and the crafted
pool meet the floors of the classes they are built for, the uniform-action fixtures meet no threshold at all (which is why the edge_*
ones exist), the counters' occupancy is the oracle's, and a one-ulp-scale nudge of the actions moves the outputs on the lattice policies."""
import os

import numpy as np
import pytest

from tests import threshold_cases as tc
from conftest import ALL_GOLDEN_FILES, load_golden

EDGE_FILES = [f for f in ALL_GOLDEN_FILES if os.path.basename(f).startswith("edge_")]
RAND_FILES = [f for f in ALL_GOLDEN_FILES if "_rand_" in os.path.basename(f)]
_name = lambda f: os.path.basename(f)[:-4]  # noqa: E731
RK, SK = 0, 0   # ProfitMax_TrPenalty_UserIncentives on V2G_profit_max_loads


def crafted_pool(n_envs=6, ports_per_cs=1, seed=5, **kw):
    from ev2gym_amd.scenario_gen import GenConfig, generate
    return tc.craft(generate(GenConfig(n_envs=n_envs, number_of_charging_stations=10, number_of_ports_per_cs=ports_per_cs, spawn_multiplier=10.0, seed=seed, **kw)))


def test_the_fixture_table_names_the_committed_files():
    assert sorted(tc.EDGE_FIXTURES) == sorted(_name(f) for f in EDGE_FILES)
    assert len(RAND_FILES) >= 20


@pytest.mark.parametrize("path", EDGE_FILES, ids=[_name(f) for f in EDGE_FILES])
def test_edge_fixture_meets_the_floors_of_its_classes(path):
    z, batch, _, _ = load_golden(path)
    pol, classes = tc.EDGE_FIXTURES[_name(path)]
    assert str(z["case"][5]) == pol
    counts = tc.count_events(z["act"][:, None, :], batch)
    nT = len(z["act"])   # the reference's mask after step t - 1 is the occupancy at step t
    if batch.uniform_ports:   # (with a topology file's port counts the reference's mask is indexed charger * n_ports + slot, not by port)
        assert np.array_equal(tc.session_at(batch)[1:nT, 0] >= 0, z["trj_mask"][:nT - 1].astype(bool)), "the counters' occupancy differs from the reference's action mask"
    tc.assert_floors(counts, classes, _name(path))


@pytest.mark.parametrize("path", RAND_FILES, ids=[_name(f) for f in RAND_FILES])
def test_uniform_actions_meet_no_threshold(path):
    z, batch, _, _ = load_golden(path)
    counts = tc.count_events(z["act"][:, None, :], batch)
    assert counts["occupied"] > 0
    assert all(counts[c] == 0 for c in tc.FLOORS), counts


def test_occupancy_is_the_oracles_action_mask():
    """session_at (the counters' occupancy) against the mask the oracle returns: the mask of step t - 1 is the occupancy at step t."""
    from oracle.oracle import Oracle
    for npc in (1, 3):
        pool = crafted_pool(ports_per_cs=npc)
        occ = tc.session_at(pool) >= 0
        ora = Oracle(pool, RK, SK)
        ora.reset()
        for t in range(pool.n_steps - 1):
            *_, mask, rc = ora.step(np.zeros((pool.n_envs, pool.n_ports)))
            assert np.array_equal(mask.astype(bool), occ[t + 1]), (npc, t)
        ora.close()


@pytest.mark.parametrize("pol,classes", [("lat32", ("key_ties",)), ("dec", ("round_ties",)), ("gate", ("edge_near", "gate_near")), ("lat64", ("round_ties",))])
@pytest.mark.parametrize("v2g", [True, False], ids=["v2g", "charge_only"])
def test_crafted_pool_meets_the_floors(pol, classes, v2g):
    pool = crafted_pool(v2g_enabled=v2g, **({} if v2g else {"cs_max_discharge_current": 0.0}))
    acts = tc.policy(pol, -1.0 if v2g else 0.0, (pool.n_steps, pool.n_envs, pool.n_ports), 3, pool)
    tc.assert_floors(tc.count_events(acts, pool), classes, f"crafted pool, {pol}")


def test_latwild_meets_the_sum_floor_on_multi_port_chargers():
    for npc in (2, 3):
        pool = crafted_pool(ports_per_cs=npc)
        acts = tc.policy("latwild", -1.0, (pool.n_steps, pool.n_envs, pool.n_ports), 4, pool)
        assert acts.min() >= -1.5 and acts.max() <= 1.5 and np.array_equal(acts * 64, np.rint(acts * 64))
        tc.assert_floors(tc.count_events(acts, pool), ("sums",), f"crafted pool, {npc} ports, latwild")


def test_the_lattice_policies_are_float32_values_and_dec_is_not():
    pool = crafted_pool()
    shape = (pool.n_steps, pool.n_envs, pool.n_ports)
    for pol in ("lat64", "lat32", "latwild"):
        a = tc.policy(pol, -1.0, shape, 1, pool)
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), pol
    a = tc.policy("dec", -1.0, shape, 1, pool)
    assert not np.array_equal(a.astype(np.float32).astype(np.float64), a)
    assert np.array_equal(np.round(tc.policy("gate", -1.0, shape, 1, pool), 5), tc.policy("gate", -1.0, shape, 1, pool))


def test_one_step_nudge_moves_the_outputs_on_the_thresholds_only():
    """Scaling ONE step's actions by 1 + 2^-40 moves that step's observation or reward by more than 1e-7 in this share of the (env, step)
    pairs of the crafted pool (printed per policy).  Uniform actions: none.  lat64: the odd numerators are exact rounding ties, the nudge takes
    the other side and the action moves by 1e-5."""
    pool = crafted_pool()
    shape = (pool.n_steps, pool.n_envs, pool.n_ports)
    moved = {pol: tc.nudge_share(pool, RK, SK, tc.policy(pol, -1.0, shape, 2, pool)) for pol in tc.POLICIES}
    moved["uniform"] = tc.nudge_share(pool, RK, SK, np.random.default_rng(2).uniform(-1.0, 1.0, shape))
    print("    share of (env, step) pairs moved by the nudge: " + ", ".join(f"{k} {v:.3f}" for k, v in moved.items()))
    assert moved["uniform"] == 0.0
    assert moved["lat64"] > 0.0
