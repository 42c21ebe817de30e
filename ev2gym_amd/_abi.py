"""ctypes mirrors of include/ev2g.h (the C-ABI structs).  Keep in sync with the header."""
import ctypes as C

ABI_VERSION = 4
COMM_ID_BYTES = 128   # EV2G_COMM_ID_BYTES = sizeof(ncclUniqueId)
LUT_LEN = 101
N_STATS = 17

REWARD_KINDS = {
    "ProfitMax_TrPenalty_UserIncentives": 0,   # rl_agent/reward.py:34-44
    "SquaredTrackingErrorReward": 1,           # rl_agent/reward.py:7-14
    "profit_maximization": 2,                  # rl_agent/reward.py:78-87
    "SqTrError_TrPenalty_UserIncentives": 3,   # rl_agent/reward.py:16-32
    "SquaredTrackingErrorRewardWithPenalty": 4,  # rl_agent/reward.py:46-58
    "SimpleReward": 5,                         # rl_agent/reward.py:60-65
    "MinimizeTrackerSurplusWithChargeRewards": 6,  # rl_agent/reward.py:67-76
    "V2G_costs_simple": 7,                     # rl_agent/reward.py:151-154
    "V2G_profitmax": 8,                        # rl_agent/reward.py:120-148
    "V2G_profitmaxV2": 9,                      # rl_agent/reward.py:156-211
    "pst_V2G_profitmaxV2": 10,                 # rl_agent/reward.py:278-339
}
STATE_KINDS = {
    "V2G_profit_max_loads": 0,                 # rl_agent/state.py:108-155
    "PublicPST": 1,                            # rl_agent/state.py:6-63
    "V2G_profit_max": 2,                       # rl_agent/state.py:65-106
}
STAT_NAMES = [  # get_statistics(), utilities/utils.py:84-101
    'total_ev_served', 'total_profits', 'total_energy_charged', 'total_energy_discharged',
    'average_user_satisfaction', 'power_tracker_violation', 'tracking_error',
    'energy_tracking_error', 'energy_user_satisfaction', 'std_energy_user_satisfaction',
    'min_energy_user_satisfaction', 'total_steps_min_emergency_battery_capacity_violation',
    'total_transformer_overload', 'battery_degradation', 'battery_degradation_calendar',
    'battery_degradation_cycling', 'total_reward']

# grid-simulation keys of the same dict (utils.py:103-112): constant 0 unless EV2GymVec(grid_statistics=True) fills the three voltage keys from the
# grid kernel's accumulators (ev2g_grid_get_stats); saved_grid_energy is 0 in the reference too
GRID_STAT_ZEROS = ('saved_grid_energy', 'voltage_violation', 'voltage_violation_counter',
                   'voltage_violation_counter_per_step')

COST_KINDS = {
    "transformer_overload_usrpenalty_cost": 1,         # rl_agent/cost.py:8-18
    "ProfitMax_TrPenalty_UserIncentives_safety": 2,    # rl_agent/cost.py:22-27
}
HEURISTIC_KINDS = {   # the env-reading heuristic agents run on the device (ev2g_heuristic_create)
    "ChargeAsLateAsPossible": 0,                    # baselines/heuristics.py:98-149
    "ChargeAsFastAsPossibleToDesiredCapacity": 1,   # baselines/heuristics.py:230-267
    "RoundRobin": 2,                                # baselines/heuristics.py:7-96
}
AGENT_KINDS = {   # every agent ev2g_heuristic_create knows: the three above and the header's EV2G_AGENT_* kinds, same number space
    **HEURISTIC_KINDS,
    "ChargeAsLateAsPossibleToDesiredCapacity": 3,   # baselines/heuristics.py:561-622
    "RoundRobin_GF": 4,                             # baselines/heuristics.py:270-399  (one port per charger)
    "RoundRobin_GF_off_allowed": 5,                 # baselines/heuristics.py:402-530  (one port per charger)
}
WRAP_KINDS = {   # the reference's action wrappers run on the device (ev2g_wrap_create), by class name
    "BinaryAction": 0,                              # rl_agent/action_wrappers.py:8-47
    "ThreeStep_Action": 1,                          # rl_agent/action_wrappers.py:50-90
    "ThreeStep_Action_DiscreteActionSpace": 1,      # rl_agent/action_wrappers.py:93-138  (the same action())
    "Rescale_RepairLayer": 2,                       # rl_agent/action_wrappers.py:159-451  (one port per charger)
}
AUTO_RESET_SAME = 1
AUTO_RESET_NEXT = 2

ERR_ARG = -1
ERR_STATE = -3
ERR_DONE = -4
ERR_OVERCURRENT = -5
FLAG_LOG_CS_HISTORY = 1
FLAG_NULL_STREAM = 2
FLAG_LOG_SOC = 4
FLAG_REFILLABLE = 8   # fixed-size session blocks per scenario: ev2g_pool_refill can re-draw scenarios on the device

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)
_pl = C.POINTER(C.c_int64)

# (field name, element ctype) of every pointer member, in header order
BATCH_ARRAYS = [
    ("cs_min_charge_current", C.c_double), ("cs_max_charge_current", C.c_double),
    ("cs_min_discharge_current", C.c_double), ("cs_max_discharge_current", C.c_double),
    ("cs_voltage", C.c_double), ("cs_phases", C.c_int32), ("cs_transformer", C.c_int32), ("cs_n_ports", C.c_int32),
    ("charge_price", C.c_double), ("discharge_price", C.c_double), ("power_setpoints", C.c_double),
    ("tr_max_power", C.c_double), ("tr_min_power", C.c_double), ("tr_inflexible_load", C.c_double),
    ("tr_solar_power", C.c_double), ("tr_load_forecast", C.c_double), ("tr_pv_forecast", C.c_double),
    ("tr_dr", C.c_double), ("tr_n_dr", C.c_int32), ("tr_steps_ahead", C.c_int32),
    ("env_session_start", C.c_int64),
    ("ev_cs", C.c_int32), ("ev_t_arr", C.c_int32), ("ev_t_dep", C.c_int32), ("ev_phases", C.c_int32),
    ("ev_lut", C.c_int32),
    ("ev_cap0", C.c_double), ("ev_B", C.c_double), ("ev_desired", C.c_double), ("ev_minB", C.c_double),
    ("ev_min_emerg", C.c_double), ("ev_pac_max", C.c_double), ("ev_pac_min", C.c_double),
    ("ev_pdis_max", C.c_double), ("ev_pdis_min", C.c_double), ("ev_ts", C.c_double), ("ev_tsm", C.c_double),
    ("ev_eta_ch", C.c_double), ("ev_eta_dis", C.c_double), ("lut", C.c_double),
]


class ScenarioBatchC(C.Structure):
    _fields_ = [
        ("n_envs", C.c_int32), ("n_steps", C.c_int32), ("timescale", C.c_int32), ("n_chargers", C.c_int32),
        ("ports_per_charger", C.c_int32), ("n_transformers", C.c_int32), ("horizon", C.c_int32),
        ("n_dr_max", C.c_int32), ("n_lut", C.c_int32), ("reserved0", C.c_int32), ("n_sessions", C.c_int64),
    ] + [(name, C.POINTER(ct)) for name, ct in BATCH_ARRAYS]


class ConfigC(C.Structure):
    _fields_ = [("device", C.c_int32), ("reward_kind", C.c_int32), ("state_kind", C.c_int32),
                ("flags", C.c_int32), ("stream", C.c_void_p), ("cost_kind", C.c_int32), ("n_active_envs", C.c_int32)]


class StepExtrasC(C.Structure):
    _fields_ = [("cost", C.c_void_p), ("cost_step_stride", C.c_int64), ("obs_f32", C.c_void_p),
                ("obs_f32_step_stride", C.c_int64), ("actions_f32", C.c_void_p)]


class OnPolicyRowsC(C.Structure):   # ev2g_onpolicy_rows: the device arrays of an ev2g_ac_collect segment, in header order
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("values", C.c_void_p), ("log_probs", C.c_void_p),
                ("reward", C.c_void_p), ("done", C.c_void_p), ("mask", C.c_void_p)]


AC_ACTIVATIONS = {"tanh": 0, "relu": 1}   # EV2G_AC_TANH (SB3's default activation_fn) / EV2G_AC_RELU
AC_MAX_IN, AC_MAX_HIDDEN, AC_MAX_OUT = 192, 256, 64   # the limits of ev2g_ac_create (EV2G_AC_MAX_*, csrc/ev2g_policy_host.h)
# The network's thirteen parameter arrays in the order of the ABI's argument lists (ac_params, csrc/ev2g_policy_host.h): the policy trunk, the
# value trunk, the action head, the value head -- weights [out, in] as torch.nn.Linear keeps them -- then log_std.
AC_PARAMS = ("pi_W1", "pi_b1", "pi_W2", "pi_b2", "vf_W1", "vf_b1", "vf_W2", "vf_b2", "action_W", "action_b", "value_W", "value_b", "log_std")


def ac_param_shapes(d_in, h1, h2, v1, v2, d_out):
    """The thirteen shapes, in AC_PARAMS' order."""
    return ((h1, d_in), (h1,), (h2, h1), (h2,), (v1, d_in), (v1,), (v2, v1), (v2,), (d_out, h2), (d_out,), (1, v2), (1,), (d_out,))


def ac_widths(weights):
    """(d_in, h1, h2, v1, v2, d_out) as the leading arrays of AC_PARAMS' order say them (the shapes are checked by GaussianActorCritic)."""
    shape = dict(zip(AC_PARAMS, (a.shape for a in weights)))
    (h1, d_in), v1 = shape["pi_W1"], shape["vf_W1"][0]
    return d_in, h1, shape["pi_W2"][0], v1, shape["vf_W2"][0], shape["action_W"][0]


class PpoConfigC(C.Structure):   # ev2g_ppo_config, in header order
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("adam_eps", C.c_double), ("clip_range", C.c_double),
                ("vf_coef", C.c_double), ("ent_coef", C.c_double), ("max_grad_norm", C.c_double), ("normalize_advantage", C.c_int32)]


class A2cConfigC(C.Structure):   # ev2g_a2c_config, in header order
    _fields_ = [("lr", C.c_double), ("alpha", C.c_double), ("rms_eps", C.c_double), ("vf_coef", C.c_double), ("ent_coef", C.c_double),
                ("max_grad_norm", C.c_double), ("normalize_advantage", C.c_int32), ("use_rms_prop", C.c_int32)]


class PpoInfoC(C.Structure):   # ev2g_ppo_info
    _fields_ = [("lds_bytes", C.c_int64), ("workspace_bytes", C.c_int64), ("grid_cap", C.c_int32), ("n_params", C.c_int32)]


class TrpoConfigC(C.Structure):   # ev2g_trpo_config, in header order
    _fields_ = [("lr", C.c_double), ("target_kl", C.c_double), ("cg_damping", C.c_double), ("line_search_shrinking_factor", C.c_double),
                ("cg_max_steps", C.c_int32), ("line_search_max_iter", C.c_int32), ("normalize_advantage", C.c_int32)]


class TrpoInfoC(C.Structure):   # ev2g_trpo_info
    _fields_ = [("lds_bytes", C.c_int64), ("workspace_bytes", C.c_int64), ("grid_cap", C.c_int32), ("n_params", C.c_int32), ("n_actor", C.c_int32)]


class TrpoReportC(C.Structure):   # ev2g_trpo_report
    _fields_ = [("cg_iterations", C.c_int32), ("line_search_tries", C.c_int32), ("accepted", C.c_int32), ("failed", C.c_int32),
                ("objective_before", C.c_double), ("objective_after", C.c_double), ("kl", C.c_double), ("beta", C.c_double), ("c", C.c_double),
                ("xHx", C.c_double)]


# the actor's seven arrays in the order of a flat TRPO vector (sb3_contrib: the parameters without "value" in their name), as indices of AC_PARAMS
TRPO_ACTOR = (12, 0, 1, 2, 3, 8, 9)


class Td3ConfigC(C.Structure):   # ev2g_td3_config, in header order
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("adam_eps", C.c_double), ("tau", C.c_double), ("gamma", C.c_double),
                ("target_policy_noise", C.c_double), ("target_noise_clip", C.c_double), ("n_critics", C.c_int32), ("policy_delay", C.c_int32)]


class ReplayRingC(C.Structure):   # ev2g_replay_ring
    _fields_ = [("n_blocks", C.c_int32), ("T", C.c_int32), ("E", C.c_int32), ("D", C.c_int32), ("P", C.c_int32), ("obs", C.c_void_p),
                ("actions", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p)]


class SacConfigC(C.Structure):   # ev2g_sac_config, in header order
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("adam_eps", C.c_double), ("tau", C.c_double), ("gamma", C.c_double),
                ("ent_coef", C.c_double), ("target_entropy", C.c_double), ("n_critics", C.c_int32), ("target_update_interval", C.c_int32),
                ("ent_coef_auto", C.c_int32), ("target_entropy_auto", C.c_int32)]


class TqcConfigC(C.Structure):   # ev2g_tqc_config, in header order: ev2g_sac_config's fields, then the two quantile settings
    _fields_ = SacConfigC._fields_ + [("n_quantiles", C.c_int32), ("top_quantiles_to_drop_per_net", C.c_int32)]


class ArsConfigC(C.Structure):   # ev2g_ars_config, in header order
    _fields_ = [("learning_rate", C.c_double), ("delta_std", C.c_double), ("alive_bonus_offset", C.c_double), ("n_delta", C.c_int32), ("n_top", C.c_int32)]


class ArsInfoC(C.Structure):   # ev2g_ars_info
    _fields_ = [("max_in", C.c_int32), ("max_hidden", C.c_int32), ("max_out", C.c_int32), ("max_delta", C.c_int32), ("n_params", C.c_int32),
                ("candidate_floats", C.c_int64), ("image_bytes", C.c_int64), ("delta_bytes", C.c_int64), ("total_bytes", C.c_int64), ("lds_bytes", C.c_int64)]


class ArsReportC(C.Structure):   # ev2g_ars_report
    _fields_ = [("sigma_r", C.c_double), ("step", C.c_double), ("iteration", C.c_int64), ("refused", C.c_int32), ("first_bad", C.c_int32), ("n_top", C.c_int32),
                ("reserved", C.c_int32)]


ARS_KINDS = {"MlpPolicy": 0, "LinearPolicy": 1}   # EV2G_ARS_MLP, EV2G_ARS_LINEAR


def ars_param_shapes(kind, d_in, h1, h2, d_out):
    """theta's arrays in parameters_to_vector order: the MLP policy's six, the linear policy's one."""
    if kind == "LinearPolicy":
        return [(d_out, d_in)]
    return [(h1, d_in), (h1,), (h2, h1), (h2,), (d_out, h2), (d_out,)]


TD3_MAX_BATCH = 1024   # EV2G_TD3_MAX_BATCH


def td3_param_shapes(d_in, h1, h2, d_out, n_critics):
    """The 6 + 6 n_critics shapes in SB3's parameter order: the actor's six arrays, then each critic's."""
    actor = [(h1, d_in), (h1,), (h2, h1), (h2,), (d_out, h2), (d_out,)]
    critic = [(h1, d_in + d_out), (h1,), (h2, h1), (h2,), (1, h2), (1,)]
    return actor + critic * int(n_critics)


def sac_param_shapes(d_in, h1, h2, d_out, n_critics):
    """The 8 + 6 n_critics shapes in SB3's parameter order: actor.latent_pi.{0,2}, actor.mu, actor.log_std (weight, bias each), then each critic's."""
    actor = [(h1, d_in), (h1,), (h2, h1), (h2,), (d_out, h2), (d_out,), (d_out, h2), (d_out,)]
    critic = [(h1, d_in + d_out), (h1,), (h2, h1), (h2,), (1, h2), (1,)]
    return actor + critic * int(n_critics)


def tqc_param_shapes(d_in, h1, h2, d_out, n_critics, n_quantiles):
    """The 8 + 6 n_critics shapes in sb3_contrib's parameter order: SAC's actor, then each quantile critic's (the last layer has n_quantiles rows)."""
    critic = [(h1, d_in + d_out), (h1,), (h2, h1), (h2,), (n_quantiles, h2), (n_quantiles,)]
    return sac_param_shapes(d_in, h1, h2, d_out, 0) + critic * int(n_critics)


TQC_MAX_CRITICS, TQC_MAX_QUANTILES, TQC_MAX_ATOMS = 5, 64, 128   # EV2G_TQC_MAX_* (csrc/ev2g_tqc.h)


PPO_STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction")   # the six statistics of ev2g_ppo_grad


class EnvViewC(C.Structure):
    _fields_ = [
        ("current_step", C.c_int32), ("n_ports", C.c_int32), ("n_chargers", C.c_int32),
        ("n_transformers", C.c_int32), ("n_steps", C.c_int32),
        ("port_capacity", _pd), ("port_energy", _pd), ("port_current", _pd), ("port_total_energy", _pd),
        ("port_required_energy", _pd), ("port_prev_power", _pd), ("port_cycles", _pi), ("port_session", _pi),
        ("cs_power", _pd), ("cs_amps", _pd), ("cs_profits", _pd), ("cs_energy_charged", _pd),
        ("cs_energy_discharged", _pd), ("tr_power", _pd), ("tr_overload", _pd), ("power_usage", _pd),
        ("power_potential", _pd), ("session_port", _pi), ("session_afap", _pd), ("session_final_cap", _pd),
    ]


# ---- scenario generator (ev2g_gen_config, include/ev2g.h) ----
GEN_INT_FIELDS = ["simulation_length", "timescale", "number_of_charging_stations", "number_of_ports_per_cs", "number_of_transformers",
                  "scenario", "simulation_days", "hour", "minute", "random_hour", "v2g_enabled", "power_setpoint_enabled",
                  "inflexible_loads", "solar_power", "demand_response", "dr_events_per_day", "dr_event_length_minutes_min",
                  "dr_event_length_minutes_max", "dr_notification_of_event_minutes", "heterogeneous_ev_specs", "fleet_with_efficiency_tables",
                  "fleet", "cs_phases", "ev_phases", "ev_min_time_of_stay", "n_ev_specs"]
GEN_DOUBLE_FIELDS = ["spawn_multiplier", "discharge_price_factor", "power_setpoint_flexiblity",
                     "inflexible_loads_capacity_multiplier_mean", "inflexible_loads_forecast_mean", "inflexible_loads_forecast_std",
                     "solar_power_capacity_multiplier_mean", "solar_power_forecast_mean", "solar_power_forecast_std",
                     "dr_event_capacity_percentage_mean", "dr_event_capacity_percentage_std", "dr_event_start_hour_mean", "dr_event_start_hour_std",
                     "transformer_max_power", "cs_min_charge_current", "cs_max_charge_current", "cs_min_discharge_current",
                     "cs_max_discharge_current", "cs_voltage", "ev_battery_capacity", "ev_max_ac_charge_power", "ev_min_ac_charge_power",
                     "ev_max_discharge_power", "ev_min_discharge_power", "ev_charge_efficiency", "ev_discharge_efficiency", "ev_transition_soc",
                     "ev_transition_soc_multiplier", "ev_min_battery_capacity", "ev_min_emergency_battery_capacity", "ev_desired_capacity"]
GEN_TOPO_INT = ["topo_n_ports", "topo_transformer", "topo_phases"]
GEN_TOPO_DOUBLE = ["topo_min_charge_current", "topo_max_charge_current", "topo_min_discharge_current", "topo_max_discharge_current",
                   "topo_voltage", "topo_tr_max_power"]
GEN_SCENARIOS = {"workplace": 0, "public": 1, "private": 2}
GEN_DAYS = {"weekdays": 0, "weekends": 1, "both": 2}
GEN_FLEETS = {"v2g2024": 0, "ev_plus_phev": 1}


GEN_SPEC_DOUBLE = ["spec_registrations", "spec_battery_capacity", "spec_max_ac_charge_power", "spec_max_ac_discharge_power", "spec_efficiency"]
GEN_TABLE_DOUBLE = ["tab_arrival_week", "tab_arrival_weekend", "tab_stay", "tab_energy", "tab_pv"]


class GenConfigC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in GEN_INT_FIELDS] + [("tr_seed", C.c_int64)] + [(n, C.c_double) for n in GEN_DOUBLE_FIELDS]
                + [(n, _pi) for n in GEN_TOPO_INT] + [(n, _pd) for n in GEN_TOPO_DOUBLE]
                + [(n, _pd) for n in GEN_SPEC_DOUBLE] + [(n, _pd) for n in GEN_TABLE_DOUBLE] + [("n_pv", C.c_int64)])
