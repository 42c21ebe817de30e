"""Host-side logic that needs no GPU: scenario batches, the vectorised generator, YAML mapping."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, GOLDEN_FILES, ROOT, load_golden
from ev2gym_amd import _abi
from ev2gym_amd.config import gen_config_from_yaml
from ev2gym_amd.scenario import ScenarioBatch, resolve_ports
from ev2gym_amd.scenario_gen import GenConfig, generate, occupancy_fraction

CFG = os.path.join(ROOT, "ev2gym_amd", "example_config_files")


def _same_25cs():
    out = []
    for f in GOLDEN_FILES:
        if os.path.basename(f).startswith("v2gppl_") and "_s" in f:
            z, b, rk, sk = load_golden(f)
            if b.n_chargers == 25 and b.ports_per_charger == 1 and b.timescale == 15 and b.arrays["cs_min_charge_current"][0] == 0:
                out.append(b)
    return out


def test_concat_select_roundtrip_and_lut_dedup():
    bs = _same_25cs()
    assert len(bs) >= 4
    cat = ScenarioBatch.concat(bs)
    assert cat.n_envs == len(bs) and cat.n_sessions == sum(b.n_sessions for b in bs)
    assert cat.n_lut <= 8   # identical efficiency tables are shared
    for i, b in enumerate(bs):
        one = cat.select([i])
        for k in ("ev_t_arr", "ev_t_dep", "ev_cap0", "ev_B", "ev_ts", "charge_price", "tr_max_power"):
            assert np.array_equal(np.asarray(one.arrays[k]).reshape(-1), np.asarray(b.arrays[k]).reshape(-1)), k
        lut_a = one.arrays["lut"][np.maximum(one.arrays["ev_lut"], 0)]
        lut_b = b.arrays["lut"][np.maximum(b.arrays["ev_lut"], 0)]
        assert np.array_equal(lut_a, lut_b)


def test_shards_partition_the_batch():
    cat = ScenarioBatch.concat(_same_25cs()).tile(11)
    parts = [cat.shard(r, 3) for r in range(3)]
    assert sum(p.n_envs for p in parts) == 11
    again = ScenarioBatch.concat(parts)
    for k in ("ev_t_arr", "ev_cap0", "env_session_start", "charge_price", "tr_dr"):
        assert np.array_equal(again.arrays[k], cat.arrays[k]), k


def test_save_load(tmp_path):
    b = generate(GenConfig.public_pst(5, 7, seed=4))
    p = str(tmp_path / "b.npz")
    b.save(p)
    c = ScenarioBatch.load(p)
    for k, v in b.arrays.items():
        assert np.array_equal(v, c.arrays[k], equal_nan=True), k


@pytest.mark.parametrize("cfg", [GenConfig.v2g_profit_plus_loads(64, 50, seed=1), GenConfig.public_pst(64, 20, seed=2),
                                 GenConfig.v2g_profit_plus_loads(8, 12, 3, seed=3, number_of_ports_per_cs=2),
                                 GenConfig.v2g_profit_plus_loads(3, 200, 10, seed=5, heterogeneous_ev_specs=False)])
def test_generator_respects_the_spawner_rules(cfg):
    b = generate(cfg)
    a = b.arrays
    T = b.n_steps
    assert (a["ev_t_arr"] >= 3).all() and (a["ev_t_dep"] > a["ev_t_arr"]).all()
    assert (a["ev_t_dep"] + 1 < T).all(), "empty_ports_at_end_of_simulation (utils.py:254-256)"
    assert (a["ev_cap0"] >= 0).all() and (a["ev_cap0"] <= a["ev_B"]).all()   # 0 happens in the reference too (B == required energy, small battery)
    assert (a["charge_price"] <= 0).all() and (a["discharge_price"] >= 0).all()
    st = a["env_session_start"]
    for e in range(b.n_envs):   # arrival order inside every env
        assert (np.diff(a["ev_t_arr"][st[e]:st[e + 1]]) >= 0).all()
    ports = resolve_ports(b)     # first-free replay never runs out of ports
    assert (ports >= 0).all()
    # a port is never double booked
    for e in range(min(b.n_envs, 8)):
        sl = slice(st[e], st[e + 1])
        for p in np.unique(ports[sl]):
            m = ports[sl] == p
            ta, td = a["ev_t_arr"][sl][m], a["ev_t_dep"][sl][m]
            assert (ta[1:] > td[:-1]).all()
    phi = occupancy_fraction(b)
    assert 0.05 < phi < 0.5
    if cfg.demand_response:
        assert (a["tr_n_dr"] == 1).all()
        assert (a["tr_max_power"].min(axis=2) < cfg.transformer_max_power).any()
    if cfg.power_setpoint_enabled:
        assert a["power_setpoints"].max() > 0


def test_generator_is_deterministic_and_seeded():
    a = generate(GenConfig.v2g_profit_plus_loads(16, 10, seed=7))
    b = generate(GenConfig.v2g_profit_plus_loads(16, 10, seed=7))
    c = generate(GenConfig.v2g_profit_plus_loads(16, 10, seed=8))
    assert all(np.array_equal(a.arrays[k], b.arrays[k], equal_nan=True) for k in a.arrays)
    assert not np.array_equal(a.arrays["ev_cap0"], c.arrays["ev_cap0"])


@pytest.mark.parametrize("name,P,R,v2g,setp", [("V2GProfitPlusLoads.yaml", 25, 1, True, False), ("PublicPST.yaml", 20, 1, False, True),
                                               ("V2GProfitPlusLoads_50cs.yaml", 50, 1, True, False),
                                               ("V2GProfitPlusLoads_1000cs_50tr.yaml", 1000, 50, True, False)])
def test_yaml_schema_maps_onto_the_generator(name, P, R, v2g, setp):
    g = gen_config_from_yaml(os.path.join(CFG, name), 2, seed=1)
    b = generate(g)
    assert (b.n_ports, b.n_transformers, b.v2g_enabled) == (P, R, v2g)
    assert (b.arrays["power_setpoints"].max() > 0) == setp
    assert b.obs_dim(_abi.STATE_KINDS["V2G_profit_max_loads"]) == 22 + 40 * R + 2 * P
    assert b.obs_dim(_abi.STATE_KINDS["PublicPST"]) == 3 + 3 * P
    if R > 1:   # round-robin charger -> transformer map (loaders.py:494-498)
        assert np.array_equal(b.arrays["cs_transformer"], np.arange(P) % R)


def test_plugin_resolution():
    from ev2gym_amd.rl_agent import reward as R, state as S
    from ev2gym_amd.vec_env import _kind
    assert _kind(S.PublicPST, _abi.STATE_KINDS, "s") == 1 and _kind("V2G_profit_max_loads", _abi.STATE_KINDS, "s") == 0
    assert _kind(R.profit_maximization, _abi.REWARD_KINDS, "r") == 2
    assert _kind(R.SimpleReward, _abi.REWARD_KINDS, "r") == 5 and _kind("V2G_profitmax", _abi.REWARD_KINDS, "r") == 8
    assert sorted(_abi.REWARD_KINDS.values()) == list(range(11))           # every fused reward has a kernel id (include/ev2g.h)
    assert _kind(lambda env: 0.0, _abi.REWARD_KINDS, "r") is None
    with pytest.raises(ValueError):
        _kind("NoSuchReward", _abi.REWARD_KINDS, "r")


@pytest.mark.parametrize("name,yaml_file", [("V2GProfitPlusLoads", "V2GProfitPlusLoads.yaml"), ("PublicPST", "PublicPST.yaml"),
                                            ("PrivateV2GPPL", "V2GProfitPlusLoads.yaml"), ("PublicPSTWeekend", "PublicPST.yaml"),
                                            ("PrivateV2GPPLWeekend", "V2GProfitPlusLoads.yaml")])
@pytest.mark.parametrize("backend", ["numpy", "native"])
def test_generator_reproduces_the_reference_spawn_statistics(name, yaml_file, backend):
    """Statistical parity of the vectorised scenario generator with the reference's EV_spawner / spawn_single_EV
    (SURVEY.md §8f-1): tests/golden/spawn_stats.json holds summary statistics of 300 reference resets per config
    (oracle/capture_spawn_stats.py); 300 generated envs must land close to them.  Tolerances are a few standard errors
    of these sample sizes plus the modelling error of hourly tables / representative fleet classes."""
    import json
    from ev2gym_amd.config import gen_config_from_yaml, load_yaml
    from ev2gym_amd.scenario_gen import generate, generate_native, occupancy_fraction
    if backend == "native":   # the library's own generator (ev2g_generate, csrc/ev2g_gen.h): same model, counter-based random numbers
        generate = generate_native
    ref = json.load(open(os.path.join(GOLDEN_DIR, "spawn_stats.json")))[name]
    cfg_dir = os.path.join(os.path.dirname(GOLDEN_DIR), "..", "ev2gym_amd", "example_config_files")
    over = {"scenario": "private"} if name.startswith("Private") else {}
    if name.endswith("Weekend"):
        over["simulation_days"] = "weekends"
    b = generate(gen_config_from_yaml({**load_yaml(os.path.join(cfg_dir, yaml_file)), **over}, 300, 11))
    a, T, P = b.arrays, b.n_steps, b.n_ports
    st = a["env_session_start"]
    stay = a["ev_t_dep"] - a["ev_t_arr"]
    soc0 = a["ev_cap0"] / a["ev_B"]
    req = a["ev_B"] - a["ev_cap0"]

    def near(x, key, rel=0.0, abs_=0.0):
        assert abs(x - ref[key]) <= rel * abs(ref[key]) + abs_, f"{key}: generator {x:.4g} vs reference {ref[key]:.4g}"
    near(occupancy_fraction(b), "occupancy_mean", rel=0.08)   # (300 envs: +-3 % sampling noise on top of the tables' few-percent modelling error)
    near(((st[1:] - st[:-1]) / P).mean(), "sessions_per_port_mean", rel=0.05)
    near(((st[1:] - st[:-1]) / P).std(), "sessions_per_port_std", rel=0.25)
    near(stay.mean(), "stay_mean", rel=0.05)
    for qn, qv in (("stay_q05", .05), ("stay_q25", .25), ("stay_q50", .5), ("stay_q75", .75), ("stay_q95", .95)):
        near(np.quantile(stay, qv), qn, abs_=4.0)
    near(soc0.mean(), "soc_at_arrival_mean", abs_=0.04)
    # the low tail is lumpy where small batteries are in the fleet (an 8 kWh PHEV arrives with an integer kWh: SoC 0.25, 0.375 ...): the
    # 10 % quantile sits on one step or the next depending on the sample (0.25 / 0.345 over six seeds of either generator; reference 0.27)
    near(np.quantile(soc0, .1), "soc_at_arrival_q10", abs_=0.08)
    near(np.quantile(soc0, .9), "soc_at_arrival_q90", abs_=0.04)
    near(req.mean(), "required_energy_mean", rel=0.08)
    near(np.quantile(req, .5), "required_energy_q50", rel=0.12)
    near(a["ev_B"].mean(), "battery_capacity_mean", rel=0.08)
    near((a["ev_B"] < 20).mean(), "small_battery_share", abs_=0.06)
    hist = np.histogram(a["ev_t_arr"], bins=np.linspace(0, T, 8))[0] / len(stay)
    assert np.abs(hist - np.array(ref["arrival_hist_7bins"])).max() <= 0.04, (hist, ref["arrival_hist_7bins"])


@pytest.mark.parametrize("backend", ["numpy", "native"])
def test_generated_power_setpoints_resemble_the_reference_ones(backend):
    """generate_power_setpoints (utils.py:664-757) is re-implemented vectorised and simplified: its output must still
    carry about the same energy relative to what the EVs need, peak, duty and level as the reference's (PublicPST)."""
    import json
    from ev2gym_amd.config import gen_config_from_yaml, load_yaml
    from ev2gym_amd.scenario_gen import generate, generate_native
    if backend == "native":
        generate = generate_native
    ref = json.load(open(os.path.join(GOLDEN_DIR, "spawn_stats.json")))["PublicPST"]
    cfg_dir = os.path.join(os.path.dirname(GOLDEN_DIR), "..", "ev2gym_amd", "example_config_files")
    b = generate(gen_config_from_yaml(load_yaml(os.path.join(cfg_dir, "PublicPST.yaml")), 300, 5))
    a, st, dt = b.arrays, b.arrays["env_session_start"], b.timescale
    ratio, peak, duty, level = [], [], [], []
    for e in range(b.n_envs):
        sp = a["power_setpoints"][e]
        need = (a["ev_B"][st[e]:st[e + 1]] - a["ev_cap0"][st[e]:st[e + 1]]).sum()
        if sp.any() and need > 0:
            ratio.append(sp.sum() * dt / 60 / need); peak.append(sp.max()); duty.append((sp > 0).mean()); level.append(sp.mean())
    assert abs(np.mean(ratio) - ref["setpoint_energy_ratio_mean"]) <= 0.12 * ref["setpoint_energy_ratio_mean"]
    assert abs(np.mean(peak) - ref["setpoint_max_mean"]) <= 0.25 * ref["setpoint_max_mean"]
    assert abs(np.mean(duty) - ref["setpoint_nonzero_fraction"]) <= 0.08
    assert abs(np.mean(level) - ref["setpoint_mean_kw"]) <= 0.15 * ref["setpoint_mean_kw"]


@pytest.mark.parametrize("yaml_file,T,P,R", [("PublicPST.yaml", 112, 20, 1), ("simplePST.yaml", 96, 2, 1), ("V2GProfitMax.yaml", 112, 25, 1),
                                             ("V2GProfitPlusLoads.yaml", 112, 25, 1), ("V2GProfitPlusLoads_50cs.yaml", 112, 50, 1),
                                             ("V2GProfitPlusLoads_1000cs_50tr.yaml", 112, 1000, 50)])
def test_every_shipped_config_generates_a_batch(yaml_file, T, P, R):
    """The example configs mirror the reference's example_config_files (PublicPST / simplePST / V2GProfitMax / V2GProfitPlusLoads) plus the
    two BASELINE shapes: each must load, generate and finalise, with the features its switches select."""
    import warnings
    from ev2gym_amd.config import gen_config_from_yaml, load_yaml
    from ev2gym_amd.scenario_gen import generate
    cfg = load_yaml(os.path.join(CFG, yaml_file))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # simplePST pins a calendar day (random_day: False): the generator says its curves are synthetic
        b = generate(gen_config_from_yaml(cfg, 6, 2))
    a = b.arrays
    assert (b.n_envs, b.n_steps, b.n_ports, b.n_transformers) == (6, T, P, R)
    assert (a["ev_t_arr"] < a["ev_t_dep"]).all() and a["ev_t_arr"].min() >= 0
    loads = bool(cfg["inflexible_loads"]["include"]); pv = bool(cfg["solar_power"]["include"])
    assert bool(np.abs(a["tr_inflexible_load"]).sum() > 0) == loads
    assert bool(np.abs(a["tr_solar_power"]).sum() > 0) == pv
    assert bool(a["power_setpoints"].any()) == bool(cfg["power_setpoint_enabled"])
    if not cfg["heterogeneous_ev_specs"]:
        assert len(np.unique(a["ev_B"])) == 1   # one EV model (ev2gym_env.py:  ev_specs are only read when heterogeneous)
    if not cfg["v2g_enabled"]:
        assert not b.v2g_enabled


# ---- the library's own generator (ev2g_generate): the C-ABI's counterpart of scenario_gen.generate ---------------------------------
def test_native_generator_shares_the_fitted_tables_with_the_numpy_one():
    """Two copies of the fitted constants exist (scenario_gen._HOURLY / _FLEET_* and csrc/ev2g_gen.h): they must be the same numbers."""
    import ctypes as C
    from ev2gym_amd import scenario_gen as sg
    from ev2gym_amd.engine import load_library
    L = load_library()
    out = (C.c_double * 24)()
    for kind, name in enumerate(["workplace", "public", "private", "public_weekend", "private_weekend"]):
        for which, key in enumerate(["rate", "stay"]):
            assert L.ev2g_gen_table(which, kind, out, 24) == 24
            assert np.array_equal(np.array(out[:24]), sg._HOURLY[name][key]), (name, key)
        assert L.ev2g_gen_table(2, kind, out, 24) == 1 and out[0] == sg._HOURLY[name]["energy"][0]
    fl = (C.c_double * 24)()
    assert L.ev2g_gen_table(3, 0, fl, 24) == 24 and np.array_equal(np.array(fl[:24]).reshape(8, 3), np.array([f[:3] for f in sg._FLEET_V2G]))
    assert L.ev2g_gen_table(4, 0, fl, 24) == 24 and np.array_equal(np.array(fl[:24]).reshape(8, 3), np.array(sg._FLEET_EV_PHEV))
    assert L.ev2g_gen_table(0, 9, out, 24) < 0 and L.ev2g_gen_table(0, 0, out, 3) < 0


def test_native_generator_is_a_pure_function_of_seed_and_scenario_index():
    """Counter-based draws: the batch does not depend on the number of threads, scenario i is the same scenario whatever n_scenarios is,
    another seed gives other scenarios; tr_seed pins the transformer side only (ev2gym_env.py:97-100)."""
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    cfg = GenConfig.v2g_profit_plus_loads(40, 12, 2, seed=9, number_of_ports_per_cs=2)
    a, b = generate_native(cfg, 1), generate_native(cfg, 5)
    assert all(np.array_equal(a.arrays[k], b.arrays[k], equal_nan=True) for k in a.arrays)
    small = generate_native(GenConfig.v2g_profit_plus_loads(7, 12, 2, seed=9, number_of_ports_per_cs=2))
    S = small.n_sessions
    assert S == a.arrays["env_session_start"][7]
    for k in ("ev_cap0", "ev_t_arr", "ev_t_dep", "ev_cs", "ev_ts"):
        assert np.array_equal(small.arrays[k], a.arrays[k][:S]), k
    for k in ("charge_price", "tr_inflexible_load", "tr_pv_forecast", "tr_dr"):
        assert np.array_equal(small.arrays[k], a.arrays[k][:7]), k
    other = generate_native(GenConfig.v2g_profit_plus_loads(40, 12, 2, seed=10, number_of_ports_per_cs=2))
    assert not np.array_equal(other.arrays["charge_price"], a.arrays["charge_price"])
    # random_hour: a start hour per SCENARIO, 5..15 (the reference draws one per reset, ev2gym_env.py:131-133): the PV peak (13:00) lands on 11 different steps
    rh = generate_native(GenConfig.v2g_profit_plus_loads(300, 6, 1, seed=3, random_hour=True))
    peaks = np.argmin(rh.arrays["tr_solar_power"][:, 0, :], axis=1)
    assert len(np.unique(peaks)) == 11 and len(np.unique(np.argmin(a.arrays["tr_solar_power"][:, 0, :], axis=1))) == 1
    p1 = generate_native(GenConfig.v2g_profit_plus_loads(6, 12, 2, seed=1, tr_seed=77))
    p2 = generate_native(GenConfig.v2g_profit_plus_loads(6, 12, 2, seed=2, tr_seed=77))
    assert np.array_equal(p1.arrays["tr_inflexible_load"], p2.arrays["tr_inflexible_load"]) and np.array_equal(p1.arrays["tr_dr"], p2.arrays["tr_dr"])
    assert not np.array_equal(p1.arrays["charge_price"], p2.arrays["charge_price"])


@pytest.mark.parametrize("yaml_file", ["PublicPST.yaml", "simplePST.yaml", "V2GProfitMax.yaml", "V2GProfitPlusLoads.yaml", "V2GProfitPlusLoads_1000cs_50tr.yaml"])
def test_native_generator_covers_the_shipped_configs_and_feeds_the_oracle(yaml_file):
    """Every shipped config through ev2g_generate: same structure as the numpy generator's batch, the constraints of the reference's
    spawner (a port is empty for at least two steps between two sessions, every EV leaves before the end), and the C oracle steps it."""
    import warnings
    from ev2gym_amd.config import gen_config_from_yaml, load_yaml
    from ev2gym_amd.scenario import resolve_ports
    from ev2gym_amd.scenario_gen import generate, generate_native
    from oracle.oracle import Oracle
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = gen_config_from_yaml(load_yaml(os.path.join(CFG, yaml_file)), 3, 4)
        b, ref = generate_native(cfg), generate(cfg)
    assert (b.n_envs, b.n_steps, b.n_ports, b.n_transformers, b.timescale) == (ref.n_envs, ref.n_steps, ref.n_ports, ref.n_transformers, ref.timescale)
    a = b.arrays
    for k, v in ref.arrays.items():
        assert a[k].dtype == v.dtype and a[k].shape[1:] == v.shape[1:], k
    assert b.n_sessions > 0 and (a["ev_t_dep"] < b.n_steps).all() and (a["ev_t_arr"] >= 3).all() and (a["ev_cap0"] <= a["ev_B"]).all()
    port, st, last = resolve_ports(b), a["env_session_start"], {}
    for e in range(b.n_envs):
        for s in range(st[e], st[e + 1]):
            if (e, port[s]) in last:
                assert a["ev_t_arr"][s] >= a["ev_t_dep"][last[(e, port[s])]] + 3
            last[(e, port[s])] = s
    for k in ("tr_inflexible_load", "tr_solar_power", "power_setpoints"):
        assert bool(np.abs(a[k]).sum() > 0) == bool(np.abs(ref.arrays[k]).sum() > 0), k
    if b.n_ports <= 60:
        ora = Oracle(b, 0 if b.v2g_enabled else 1, 0 if b.v2g_enabled else 1)
        ora.reset()
        for t in range(b.n_steps):
            o, r, d, m, rc = ora.step(np.ones((b.n_envs, b.n_ports)))
            assert rc == 0 and np.isfinite(o).all() and np.isfinite(r).all()
        assert d.all()
        ora.close()


@pytest.mark.parametrize("case", range(12))
def test_native_and_numpy_generators_agree_on_structure_for_random_configs(case):
    """Random corners of the config surface (timescales, start times, weekend days, two events per day, homogeneous specs, pinned transformer
    seed, multi-port chargers, several transformers): both generators accept them, produce the same static parts and shapes, respect the
    spawner's constraints, and land close to each other in the aggregate (sessions per port, mean stay, mean arrival SoC, load level)."""
    from ev2gym_amd.scenario import resolve_ports
    from ev2gym_amd.scenario_gen import GenConfig, generate, generate_native
    rng = np.random.default_rng(4000 + case)
    dt = int(rng.choice([5, 15, 30]))
    kw = dict(n_envs=160, timescale=dt, simulation_length=int(rng.choice([96, 112, 150])) if dt != 5 else 96,
              number_of_charging_stations=int(rng.integers(3, 14)), number_of_ports_per_cs=int(rng.choice([1, 1, 2, 3])),
              number_of_transformers=int(rng.integers(1, 4)), scenario=str(rng.choice(["workplace", "public", "private"])),
              simulation_days=str(rng.choice(["weekdays", "weekends", "both"])), hour=int(rng.integers(4, 12)), minute=int(rng.choice([0, 15, 30])),
              random_hour=bool(rng.random() < 0.2), spawn_multiplier=float(rng.choice([5, 10, 20])), v2g_enabled=bool(rng.random() < 0.6),
              power_setpoint_enabled=bool(rng.random() < 0.5), inflexible_loads=bool(rng.random() < 0.7), solar_power=bool(rng.random() < 0.7),
              demand_response=bool(rng.random() < 0.7), dr_events_per_day=int(rng.integers(1, 3)), dr_event_length_minutes_min=60,
              dr_event_length_minutes_max=int(rng.choice([60, 120])), tr_seed=int(rng.choice([-1, 9])),
              heterogeneous_ev_specs=bool(rng.random() < 0.7), fleet_with_efficiency_tables=bool(rng.random() < 0.5),
              fleet=str(rng.choice(["v2g2024", "ev_plus_phev"])), ev_min_time_of_stay=int(rng.choice([60, 120, 180])), seed=case)
    cfg = GenConfig(**kw)
    a, b = generate(cfg), generate_native(cfg)
    assert (a.n_envs, a.n_steps, a.n_ports, a.n_chargers, a.n_transformers, a.timescale, a.v2g_enabled) == \
           (b.n_envs, b.n_steps, b.n_ports, b.n_chargers, b.n_transformers, b.timescale, b.v2g_enabled)
    for k in a.arrays:
        assert a.arrays[k].dtype == b.arrays[k].dtype and a.arrays[k].shape[1:] == b.arrays[k].shape[1:], k
        if k.startswith("cs_"):
            assert np.array_equal(a.arrays[k], b.arrays[k]), k
    for batch in (a, b):
        x, T = batch.arrays, batch.n_steps
        if batch.n_sessions:
            assert (x["ev_t_arr"] >= 3).all() and (x["ev_t_dep"] < T).all() and (x["ev_t_dep"] - x["ev_t_arr"] >= 2).all()
            assert (x["ev_cap0"] >= 0).all() and (x["ev_cap0"] <= x["ev_B"]).all() and (x["ev_pdis_max"] <= 0).all()   # (an 8 kWh plug-in hybrid that asks for 8 kWh arrives empty, as in spawn_single_EV)
            port, st, last = resolve_ports(batch), x["env_session_start"], {}   # (raises when a charger has no free port for an arrival)
            for e in range(batch.n_envs if cfg.number_of_ports_per_cs == 1 else 0):
                # single-port chargers: the port the spawner drew IS the port the EV gets, so its 3-step-empty rule is visible here; on
                # multi-port chargers the first-free rule (ev_charger.py:266-286) may hand a just-freed port to an EV drawn for another one
                for s_ in range(st[e], st[e + 1]):
                    if (e, port[s_]) in last:
                        assert x["ev_t_arr"][s_] >= x["ev_t_dep"][last[(e, port[s_])]] + 3
                    last[(e, port[s_])] = s_
        assert (x["tr_max_power"] >= x["tr_inflexible_load"] - 1e-9).all() and (x["tr_solar_power"] <= 0).all()
        assert (x["charge_price"] < 0).all() and np.allclose(x["discharge_price"], -x["charge_price"] * cfg.discharge_price_factor)
        assert (x["power_setpoints"] >= 0).all() and bool(x["power_setpoints"].any()) == bool(cfg.power_setpoint_enabled and batch.n_sessions > 0)
    if cfg.random_hour:
        return   # the two draw their start hour from different streams: the aggregates below compare like with like only otherwise
    na, nb = a.n_sessions / (a.n_envs * a.n_ports), b.n_sessions / (b.n_envs * b.n_ports)
    assert abs(na - nb) <= 0.12 * max(na, nb) + 0.03, (na, nb)
    if min(a.n_sessions, b.n_sessions) > 300:
        sa, sb = (a.arrays["ev_t_dep"] - a.arrays["ev_t_arr"]).mean(), (b.arrays["ev_t_dep"] - b.arrays["ev_t_arr"]).mean()
        assert abs(sa - sb) <= 0.08 * sb + 0.5, (sa, sb)
        ca, cb = (a.arrays["ev_cap0"] / a.arrays["ev_B"]).mean(), (b.arrays["ev_cap0"] / b.arrays["ev_B"]).mean()
        assert abs(ca - cb) <= 0.04, (ca, cb)
    if cfg.inflexible_loads:
        assert abs(a.arrays["tr_inflexible_load"].mean() - b.arrays["tr_inflexible_load"].mean()) <= 0.06 * a.arrays["tr_inflexible_load"].mean()


def test_native_generator_takes_a_topology_and_refuses_bad_input():
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    topo = dict(n_ports=np.array([3, 2, 2, 1]), transformer=np.array([0, 0, 1, 1]), phases=np.array([3, 3, 1, 3]),
                min_charge_current=np.zeros(4), max_charge_current=np.array([32., 16., 16., 32.]), min_discharge_current=np.zeros(4),
                max_discharge_current=np.array([-32., 0., -16., -32.]), voltage=np.array([400., 230., 230., 400.]), tr_max_power=np.array([80., 60.]))
    b = generate_native(GenConfig(n_envs=5, seed=2, spawn_multiplier=10, scenario="public", topology=topo))
    assert (b.n_chargers, b.n_ports, b.n_transformers, b.ports_per_charger) == (4, 8, 2, 3)
    assert np.array_equal(b.arrays["cs_n_ports"], topo["n_ports"]) and np.array_equal(b.arrays["cs_max_discharge_current"], topo["max_discharge_current"])
    assert (b.arrays["tr_max_power"][:, 1] <= 60.0 + 1e-9).all() and b.arrays["ev_cs"].max() <= 3
    with pytest.raises(ValueError):
        generate_native(GenConfig(n_envs=2, scenario="mall"))
    with pytest.raises(EngineError):
        generate_native(GenConfig(n_envs=2, simulation_length=3))


# ---- topology files and the rest of the YAML schema (ADVICE: no key is dropped silently) -----------------------------------
def _write_topology(path, spec):
    """spec = [(transformer max_power, [n_ports of its chargers])], in the layout of example_config_files/charging_topology_10.json."""
    import json
    topo, k = {}, 0
    for i, (mp, nps) in enumerate(spec):
        chs = {}
        for n in nps:
            chs[f"charger_{k + 1}"] = dict(id=k, min_charge_current=6, max_charge_current=32 if k % 2 else 16, min_discharge_current=0,
                                           max_discharge_current=-32 if k % 2 else -16, voltage=230 if k % 2 else 400, n_ports=n,
                                           charger_type="AC", phases=1 if k == 2 else 3)
            k += 1
        topo[f"transformer_{i + 1}"] = dict(id=i + 1, max_power=mp, charging_stations=chs)
    json.dump(topo, open(path, "w"))


def _yaml(name, **over):
    import yaml
    c = yaml.load(open(os.path.join(ROOT, "ev2gym_amd", "example_config_files", name)), Loader=yaml.FullLoader)
    for k, v in over.items():
        if isinstance(v, dict):
            c[k] = {**c[k], **v}
        else:
            c[k] = v
    return c


def test_topology_file_gives_chargers_their_own_ports_and_limits(tmp_path):
    """charging_network_topology (ev2gym_env.py:176-186; loaders.py:259-276, 312-340): number of transformers / chargers, each
    charger's transformer, port count, current limits, voltage and phases come from the file; ports are numbered cumulatively."""
    tp = str(tmp_path / "topology.json")
    _write_topology(tp, [(60, [3, 2]), (40, [2, 1, 1])])
    b = generate(gen_config_from_yaml(_yaml("V2GProfitPlusLoads.yaml", charging_network_topology=tp, spawn_multiplier=10), 6, seed=3))
    a = b.arrays
    assert (b.n_chargers, b.n_transformers, b.ports_per_charger, b.n_ports, b.uniform_ports) == (5, 2, 3, 9, False)
    assert a["cs_n_ports"].tolist() == [3, 2, 2, 1, 1] and a["cs_transformer"].tolist() == [0, 0, 1, 1, 1]
    assert a["cs_max_charge_current"].tolist() == [16, 32, 16, 32, 16] and a["cs_voltage"].tolist() == [400, 230, 400, 230, 400]
    assert a["cs_phases"].tolist() == [3, 3, 1, 3, 3] and b.port_base.tolist() == [0, 3, 5, 7, 8, 9]
    assert a["tr_max_power"][:, 0].max() == 60 and a["tr_max_power"][:, 1].max() == 40
    port = resolve_ports(b)
    assert ((port >= b.port_base[a["ev_cs"]]) & (port < b.port_base[a["ev_cs"] + 1])).all()
    assert b.obs_dim(_abi.STATE_KINDS["V2G_profit_max_loads"]) == 22 + 40 * 2 + 2 * 9
    # save / load / select / concat keep the per-charger port counts
    b.save(str(tmp_path / "b.npz"))
    assert ScenarioBatch.load(str(tmp_path / "b.npz")).arrays["cs_n_ports"].tolist() == [3, 2, 2, 1, 1]
    assert ScenarioBatch.concat([b.select([0, 1]), b.select([4])]).n_ports == 9
    # a file that is not there: the reference prints "Did not find file" and carries on with the YAML's chargers (ev2gym_env.py:182-186)
    with pytest.warns(UserWarning, match="Did not find file"):
        g = gen_config_from_yaml(_yaml("V2GProfitPlusLoads.yaml", charging_network_topology=str(tmp_path / "nope.json")), 2)
    assert g.topology is None and g.number_of_charging_stations == 25


def test_yaml_keys_are_passed_through_or_reported():
    base = dict(inflexible_loads=dict(inflexible_loads_capacity_multiplier_mean=0.5, forecast_mean=50, forecast_std=0),
                solar_power=dict(solar_power_capacity_multiplier_mean=2, forecast_mean=10, forecast_std=0),
                demand_response=dict(events_per_day=3, event_capacity_percentage_mean=60, event_capacity_percentage_std=0,
                                     event_length_minutes_min=30, event_length_minutes_max=90, event_start_hour_mean=10,
                                     event_start_hour_std=1, notification_of_event_minutes=30), minute=30, tr_seed=77)
    g = gen_config_from_yaml(_yaml("V2GProfitPlusLoads.yaml", **base), 8, seed=1)
    assert (g.dr_events_per_day, g.dr_notification_of_event_minutes, g.minute, g.tr_seed) == (3, 30, 30, 77)
    b = generate(g)
    a = b.arrays
    assert a["tr_dr"].shape == (8, 1, 3, 3) and (a["tr_n_dr"] == 3).all() and (a["tr_steps_ahead"] == 2).all()
    ln = (a["tr_dr"][..., 1] - a["tr_dr"][..., 0]) * b.timescale
    assert ln.min() >= 30 and ln.max() <= 90
    assert np.allclose(a["tr_load_forecast"][:, :, 1:], np.clip(0.5 * a["tr_inflexible_load"], a["tr_min_power"], a["tr_max_power"])[:, :, 1:])
    assert np.allclose(a["tr_pv_forecast"][:, :, 1:], 0.1 * a["tr_solar_power"][:, :, 1:])
    # tr_seed: the transformer side is the same for every scenario seed (ev2gym_env.py:97-100), the EV side is not
    b2 = generate(gen_config_from_yaml(_yaml("V2GProfitPlusLoads.yaml", **base), 8, seed=2))
    assert np.array_equal(b2.arrays["tr_inflexible_load"], a["tr_inflexible_load"]) and np.array_equal(b2.arrays["tr_dr"], a["tr_dr"])
    assert not np.array_equal(b2.arrays["ev_t_arr"][:20], a["ev_t_arr"][:20])
    with pytest.raises(ValueError, match="scenario"):
        gen_config_from_yaml(_yaml("V2GProfitPlusLoads.yaml", scenario="campus"), 2)
    with pytest.raises(ValueError, match="scenario"):
        generate(GenConfig(n_envs=2, scenario="campus"))
    with pytest.raises(ValueError, match="simulation_days"):
        generate(gen_config_from_yaml(_yaml("PublicPST.yaml", simulation_days="sundays"), 2))
    wk = generate(gen_config_from_yaml(_yaml("V2GProfitPlusLoads.yaml", simulation_days="weekends"), 4, seed=3))   # workplaces: weekdays anyway
    wd = generate(gen_config_from_yaml(_yaml("V2GProfitPlusLoads.yaml"), 4, seed=3))
    assert np.array_equal(wk.arrays["ev_t_arr"], wd.arrays["ev_t_arr"])
    both = generate(gen_config_from_yaml(_yaml("PublicPST.yaml", simulation_days="both"), 64, seed=3))
    assert both.n_sessions > 0
    with pytest.raises(NotImplementedError, match="simulate_grid"):
        gen_config_from_yaml(_yaml("PublicPST.yaml", simulate_grid=True), 2)
    with pytest.warns(UserWarning, match="calendar"):
        gen_config_from_yaml(_yaml("PublicPST.yaml", random_day=False), 2)
    h = {generate(gen_config_from_yaml(_yaml("PublicPST.yaml", random_hour=True), 2, seed=s)).arrays["charge_price"][0, 0] for s in range(6)}
    assert len(h) > 1


# ---- the batched evaluation loop (evaluator.py:102-109,248-287) -----------------------------------------------------------------
class _OracleBackedEngine:
    """Test stand-in for ev2gym_amd.engine.Engine on a box without a GPU (the calls ev2gym_amd.evaluator makes), served by the CPU oracle."""

    class _Buf:
        def __init__(self, shape):
            self.a = np.zeros(shape)

        def upload(self, arr):
            self.a[...] = arr
            return self

    def __init__(self, batch, rk, sk):
        from oracle.oracle import Oracle
        self.ora, self.E, self.P, self.T = Oracle(batch, rk, sk), batch.n_envs, batch.n_ports, batch.n_steps

    def empty(self, shape, dtype=np.float64):
        return self._Buf(shape)

    def fill_uniform(self, dst, n, seed, lo, hi):
        from ev2gym_amd.engine import host_uniform
        dst.a[...] = host_uniform(n, seed, lo, hi).reshape(dst.a.shape)

    def reset(self):
        self.ora.reset()

    def step_n(self, k, acts, stride, auto_reset=0, persistent=True):
        for t in range(k):
            self.ora.step((acts.a[t] if stride else acts.a).copy())

    def stats(self):
        return self.ora.stats()

    def check_faults(self):
        pass

    def last_step_n_kernel_ms(self):
        return 0.0

    def close(self):
        self.ora.close()


def test_batched_evaluator_builds_the_reference_results_table():
    """ev2gym_amd.evaluator.evaluate: one row per (run, algorithm) with the reference's columns; the values are the terminal statistics of an
    episode driven by that algorithm's action source (checked against a plain oracle loop).  The HIP engine is replaced by an oracle-backed
    stand-in here; tests/test_python_surface_gpu.py runs the same call on the device."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import host_uniform
    from ev2gym_amd.evaluator import ALGORITHMS, RESULT_STATS, evaluate
    from ev2gym_amd.scenario_gen import GenConfig, generate
    from oracle.oracle import Oracle
    batch = generate(GenConfig.v2g_profit_plus_loads(4, 8, 1, seed=12))
    df = evaluate(batch, engine_factory=_OracleBackedEngine, seed=5, discharge_price_factor=1.0)
    assert list(df.columns) == ["run", "Algorithm", "control_horizon", "discharge_price_factor"] + RESULT_STATS + ["total_reward", "time"]
    assert len(df) == 4 * len(ALGORITHMS) and sorted(df["Algorithm"].unique()) == sorted(ALGORITHMS)
    T, E, P = batch.n_steps, batch.n_envs, batch.n_ports
    sources = {"ChargeAsFastAsPossible": np.ones((T, E, P)), "DoNothing": np.zeros((T, E, P)),
               "RandomAgent": host_uniform(T * E * P, 5, -1.0, 1.0).reshape(T, E, P)}
    for name, acts in sources.items():
        ora = Oracle(batch, 0, 0)
        ora.reset()
        for t in range(T):
            ora.step(acts[t].copy())
        st = ora.stats()
        ora.close()
        sub = df[df["Algorithm"] == name].sort_values("run")
        for k in RESULT_STATS + ["total_reward"]:
            assert np.allclose(sub[k].to_numpy(), st[:, _abi.STAT_NAMES.index(k)], rtol=0, atol=0, equal_nan=True), (name, k)
    assert (df[df["Algorithm"] == "DoNothing"]["total_energy_charged"] == 0).all()
    assert (df[df["Algorithm"] == "ChargeAsFastAsPossible"]["total_energy_charged"] > 0).all()
    with pytest.raises(NotImplementedError):
        evaluate(batch, algorithms=["RoundRobin"], engine_factory=_OracleBackedEngine)


@pytest.mark.parametrize("backend", ["numpy", "native"])
def test_demand_response_window_before_the_simulation_start_follows_python_slice_semantics(backend):
    """transformer.py:118-131 applies an event with `max_power[start:end]`: with the simulation starting at 15:00 and the event at
    12:00-13:00 both bounds are negative (-12, -8 at 15-minute steps) and select the steps T-12 .. T-9 -- the END of the episode --
    while (-2, 2) selects nothing.  Both generators reproduce that, and record the raw bounds."""
    from ev2gym_amd.scenario_gen import generate_native
    gen = generate if backend == "numpy" else generate_native
    kw = dict(hour=15, dr_event_start_hour_std=0.0, dr_event_capacity_percentage_std=0.0, inflexible_loads=False, solar_power=False)
    b = gen(GenConfig.v2g_profit_plus_loads(4, 6, seed=3, dr_event_start_hour_mean=12.0, **kw))
    T, cap = b.n_steps, 100.0
    mp, dr = b.arrays["tr_max_power"], b.arrays["tr_dr"]
    assert (dr[..., 0] == -12).all() and (dr[..., 1] == -8).all()
    assert (mp[:, :, T - 12:T - 8] == pytest.approx(cap * 0.65)) and (mp[:, :, :T - 12] == cap).all() and (mp[:, :, T - 8:] == cap).all()
    b = gen(GenConfig.v2g_profit_plus_loads(4, 6, seed=3, dr_event_start_hour_mean=14.5, **kw))   # bounds (-2, 2): an empty slice
    assert (b.arrays["tr_dr"][..., 0] == -2).all() and (b.arrays["tr_dr"][..., 1] == 2).all() and (b.arrays["tr_max_power"] == cap).all()


def test_native_generator_survives_a_request_it_cannot_allocate():
    """ev2g_generate must hand an error code back (no exception crosses the C-ABI, worker threads included): a batch far beyond
    the memory the process may use is refused, and the library keeps working afterwards.  Run in a child process whose address space
    is capped 8 GB above what it maps once the library is loaded (RLIMIT_AS): whether the request fails must not depend on how much
    RAM the host has or how it overcommits -- a host that grants it would fill the 1.9 TB batch instead."""
    import subprocess
    import sys
    code = f"""if True:
        import ctypes as C, resource, sys
        sys.path.insert(0, {ROOT!r})
        from ev2gym_amd import _abi
        from ev2gym_amd.engine import load_library
        L = load_library()
        vm = int([l.split()[1] for l in open("/proc/self/status") if l.startswith("VmSize:")][0]) * 1024
        hard = resource.getrlimit(resource.RLIMIT_AS)[1]
        cap = vm + 8 * 2**30
        resource.setrlimit(resource.RLIMIT_AS, (cap if hard == resource.RLIM_INFINITY else min(cap, hard), hard))
        cfg = _abi.GenConfigC()
        assert L.ev2g_gen_default_config(0, C.byref(cfg)) == 0
        cfg.number_of_charging_stations = 1000
        cfg.number_of_transformers = 50
        out = C.c_void_p()
        rc = L.ev2g_generate(C.byref(cfg), 2**31 - 1, 1, 8, C.byref(out))   # the first array alone (prices, [M, T] float64) would be 1.9 TB
        assert rc != 0 and not out.value, rc
        assert L.ev2g_generate(C.byref(cfg), 2, 1, 2, C.byref(out)) == 0 and out.value
        L.ev2g_gen_free(out)
        print("ok")
    """
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-2000:])


def _write_data_dir(d, scenario_cols=("private", "public", "workplace")):
    """A small EV2Gym-style data directory (the file names and layouts of ev2gym/data, synthetic numbers)."""
    import csv
    q = [f"{m // 60:02d}:{m % 60:02d}" for m in range(0, 1440, 15)]
    for name, vals in (("distribution-of-arrival.csv", lambda i: 3.0 if 32 <= i < 44 else 0.0),        # arrivals only 08:00-10:59
                       ("distribution-of-arrival-weekend.csv", lambda i: 1.0)):
        with open(os.path.join(d, name), "w", newline="", encoding="utf-8-sig") as f:
            w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
            cols = scenario_cols if "weekend" not in name else scenario_cols[:2]
            w.writerow(["Arrival time", *cols])
            for i, t in enumerate(q):
                w.writerow([t] + [vals(i)] * len(cols))
    h = [f"{m // 60:02d}:{m % 60:02d}" for m in range(0, 1440, 30)]
    for name, v in (("mean-session-length-per.csv", 4.0), ("mean-demand-per-arrival.csv", 20.0)):
        with open(os.path.join(d, name), "w", newline="", encoding="utf-8-sig") as f:
            w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
            w.writerow(["Arrival Time", "home", "public", "work"])
            for t in h:
                w.writerow([t, v, v, v])
    with open(os.path.join(d, "pv_netherlands.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["time", "local_time", "electricity"])
        for i in range(8760):
            w.writerow([f"h{i}", f"h{i}", 0.5 if 10 <= i % 24 < 14 else 0.0])    # sun between 10:00 and 13:59 every day


@pytest.mark.parametrize("backend", ["numpy", "native"])
def test_ev_specs_file_named_by_the_yaml_is_read(tmp_path, backend):
    """loaders.py:25-41: the fleet comes from the JSON `ev_specs_file` names.  A two-model file must give exactly those two
    batteries / powers (in the registrations' proportions), the efficiency table where the model has one and a scalar where it has
    not, the discharge power as written; a path that cannot be read is an error -- except for the three files EV2Gym ships, whose
    built-in stand-in fleets still meet the reference's spawn statistics (the tests above)."""
    import json
    from ev2gym_amd.config import gen_config_from_yaml, load_yaml
    from ev2gym_amd.scenario_gen import generate_native
    gen = generate if backend == "numpy" else generate_native
    spec = {"Tiny": {"number_of_registrations": 300, "battery_capacity": 21.5, "max_ac_charge_power": 3.7, "max_ac_discharge_power": 0,
                     "max_dc_charge_power": 50},
            "Big": {"number_of_registrations": 100, "battery_capacity": 88.0, "max_ac_charge_power": 22, "max_ac_discharge_power": 11,
                    "max_dc_charge_power": 150, "ch_current": [6, 16, 32], "3ph_ch_efficiency": [80, 0, 95]}}
    path = str(tmp_path / "my_fleet.json")
    json.dump(spec, open(path, "w"))
    y = {**load_yaml(os.path.join(CFG, "V2GProfitPlusLoads.yaml")), "ev_specs_file": path}
    b = gen(gen_config_from_yaml(y, 200, 5))
    a = b.arrays
    assert set(np.unique(a["ev_B"])) == {21.5, 88.0} and set(np.unique(a["ev_pac_max"])) == {3.7, 22.0}
    big = a["ev_B"] == 88.0
    assert abs(big.mean() - 0.25) < 0.03
    assert (a["ev_pdis_max"][big] == -11.0).all() and (a["ev_pdis_max"][~big] == 0).all()
    assert b.n_lut == 1 and (a["ev_lut"][big] == 0).all() and (a["ev_lut"][~big] == -1).all()
    assert np.isnan(a["ev_eta_ch"][big]).all() and ((a["ev_eta_ch"][~big] >= 0.95) & (a["ev_eta_ch"][~big] <= 1.0)).all()
    lut = a["lut"][0]   # nearest level with a non-zero efficiency (utils.py:279-288): the 16 A entry is 0 in the file.  The reference fills
    # its dict IN PLACE, level by level, so a level filled a moment ago is the nearest candidate of the next: 80 walks right up to 30 A (31 A ties 30 with 32, and 32 is the earlier key)
    assert lut[6] == 80 and lut[0] == 80 and lut[16] == 80 and lut[19] == 80 and lut[20] == 80 and lut[30] == 80 and lut[31] == 95 and lut[32] == 95 and lut[100] == 95
    with pytest.raises(FileNotFoundError):
        gen_config_from_yaml({**y, "ev_specs_file": str(tmp_path / "no_such_fleet.json")}, 2, 1)
    g = gen_config_from_yaml({**y, "ev_specs_file": "./ev2gym/data/ev_specs_v2g_enabled2024.json"}, 2, 1)   # shipped name, file absent: stand-in
    assert g.ev_specs is None and g.fleet == "v2g2024" and g.fleet_with_efficiency_tables


def test_ev_specs_efficiency_curve_is_filled_like_the_reference_fills_it(tmp_path):
    """utils.py:279-286 mutates the level dict while walking 0..100: interior zeros and wide gaps take the LEFT neighbour's value
    (a tie between an original level and one filled earlier goes to the earlier key in insertion order), non-integer levels stay
    keys that no integer current reads.  Expected values worked out by hand from that loop."""
    import json
    from ev2gym_amd.config import load_ev_specs
    spec = {"M": {"number_of_registrations": 1, "battery_capacity": 50, "max_ac_charge_power": 11, "max_ac_discharge_power": 0,
                  "ch_current": [12, 14, 16, 18, 20, 40.5], "3ph_ch_efficiency": [90, 0, 0, 0, 95, 70]}}
    path = str(tmp_path / "gaps.json")
    json.dump(spec, open(path, "w"))
    eff = load_ev_specs(path)["efficiency"][0]
    assert (eff[:20] == 90).all()          # 0..11 from 12; 13..18 hand the 90 on; 19 ties 18 (filled, earlier key) with 20 -> 18's 90
    assert eff[20] == 95 and (eff[21:40] == 95).all()
    assert eff[40] == 70 and (eff[40:] == 70).all()   # 40: |40.5 - 40| < |39 - 40| -> the 40.5 A level's 70; from there 70 walks on


@pytest.mark.parametrize("backend", ["numpy", "native"])
def test_data_dir_tables_replace_the_fitted_ones(tmp_path, backend):
    """`data_dir=` (an EV2Gym install's ev2gym/data): arrivals follow distribution-of-arrival*.csv by quarter hour, stays / required
    energy the half-hourly means (utils.py:199-233,505-528), PV the smoothed pv_netherlands.csv window (loaders.py:165-224)."""
    from ev2gym_amd.config import gen_config_from_yaml, load_yaml
    from ev2gym_amd.scenario_gen import generate_native
    gen = generate if backend == "numpy" else generate_native
    _write_data_dir(str(tmp_path))
    y = {**load_yaml(os.path.join(CFG, "V2GProfitPlusLoads.yaml")), "scenario": "public", "demand_response": {"include": False},
         "ev": {**load_yaml(os.path.join(CFG, "V2GProfitPlusLoads.yaml"))["ev"], "min_time_of_stay": 60}}
    g = gen_config_from_yaml(y, 300, 9, data_dir=str(tmp_path))
    assert g.data_tables is not None and g.data_tables["arrival_week"][33] == 3.0 and len(g.data_tables["pv"]) == 8760
    b = gen(g)
    a, T, dt = b.arrays, b.n_steps, b.timescale
    # the simulation starts at 05:00: arrivals are possible only at spawn steps in 08:00-10:59 -> t_arr (= spawn step + 1) in 13..24
    assert a["ev_t_arr"].min() >= 13 and a["ev_t_arr"].max() <= 24
    stay_h = (a["ev_t_dep"] - a["ev_t_arr"]) * dt / 60
    assert abs(stay_h.mean() - 4.5) < 0.3          # N(4 h, 0.8 h) + 1 step + 2 steps to the departure (utils.py:236-262)
    assert abs((a["ev_B"] - a["ev_cap0"]).mean() - 19.0) < 2.5   # N(20, 10) kWh, short of it where the battery is smaller
    sol = -a["tr_solar_power"][:, 0, :]
    sun_steps = np.arange(T)[(sol > 0.01 * sol.max()).any(axis=0)]
    assert sun_steps.min() >= (10 - 5) * 4 and sun_steps.max() <= (14 - 5) * 4 + 14 and sol.max() > 20   # 10:00-14:00 plus the smoothing tail (rolling + exponentially weighted mean)
    with pytest.raises(FileNotFoundError):
        gen_config_from_yaml(y, 2, 1, data_dir=str(tmp_path / "missing"))


def test_sorting_a_pool_by_busy_window_keeps_the_scenarios_and_groups_similar_ones():
    """ScenarioBatch.sorted_by_busy_window (co-scheduling for the step kernel's workgroups): a permutation of the scenarios inside every
    window, first arrivals non-decreasing inside a window, and the span a group of four neighbours is busy for shrinks."""
    b = generate(GenConfig.v2g_profit_plus_loads(96, 50, 1, seed=4))
    s = b.sorted_by_busy_window(48)
    f0, l0 = b.busy_window()
    f1, l1 = s.busy_window()
    for w in (slice(0, 48), slice(48, 96)):
        assert sorted(zip(f0[w].tolist(), l0[w].tolist())) == sorted(zip(f1[w].tolist(), l1[w].tolist()))
        assert (np.diff(f1[w]) >= 0).all()
    assert np.array_equal(np.sort(b.arrays["ev_B"]), np.sort(s.arrays["ev_B"])) and b.n_sessions == s.n_sessions
    span = lambda f, l: (l.reshape(-1, 4).max(1) - f.reshape(-1, 4).min(1) + 1).sum()
    assert span(f1, l1) < span(f0, l0)
    e = generate(GenConfig.v2g_profit_plus_loads(4, 3, 1, seed=1, spawn_multiplier=0))   # no EV at all: first = T, last = -1
    fe, le = e.busy_window()
    assert (fe == e.n_steps).all() and (le == -1).all() and e.sorted_by_busy_window().n_envs == 4
