"""ctypes host binding of libev2g_hip.so (include/ev2g.h).  The thin layer between the Python surface
(`EV2GymVec`, `EV2Gym` facade) and the HIP kernels; there is no CPU fallback: importing works anywhere,
creating an engine without the built library or without a GPU raises.

Reference boundary being replaced: ev2gym.models.ev2gym_env.EV2Gym (reset :243-331, step :333-447).
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import Optional

import numpy as np

from . import _abi
from .scenario import ScenarioBatch

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libev2g_hip.so")
_lib = None


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[ev2g {code}] {msg}")
        self.code = code


def load_library(path: Optional[str] = None):
    """dlopen libev2g_hip.so and declare the prototypes.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("EV2G_LIB") or _LIB_PATH   # EV2G_LIB: A/B builds of the library (tools/ab_bench.py)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME).  If ours were loaded
    # first from /opt/rocm, torch would later bring up a second runtime and fail with "No HIP GPUs are available";
    # importing torch first makes the dynamic linker resolve our DT_NEEDED libamdhip64.so.7 to torch's copy.
    if os.environ.get("EV2G_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise EngineError(-2, f"{path} not found: build it with `python -m ev2gym_amd.build` "
                              "(hipcc --offload-arch=gfx950); the step engine has no CPU fallback")
    L = C.CDLL(path)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    protos = {
        "ev2g_abi_version": (C.c_int, []),
        "ev2g_create": (C.c_int, [C.POINTER(_abi.ConfigC), C.POINTER(vp)]),
        "ev2g_destroy": (None, [vp]),
        "ev2g_last_error": (C.c_char_p, [vp]),
        "ev2g_load_scenarios": (C.c_int, [vp, C.POINTER(_abi.ScenarioBatchC)]),
        "ev2g_n_envs": (C.c_int, [vp]), "ev2g_n_scenarios": (C.c_int, [vp]), "ev2g_n_ports": (C.c_int, [vp]), "ev2g_obs_dim": (C.c_int, [vp]),
        "ev2g_n_steps": (C.c_int, [vp]), "ev2g_current_step": (C.c_int, [vp]),
        "ev2g_reset": (C.c_int, [vp, vp]),
        "ev2g_reset_ex": (C.c_int, [vp, vp, i64]),
        "ev2g_scenario_offset": (i64, [vp]),
        "ev2g_set_step_extras": (C.c_int, [vp, C.POINTER(_abi.StepExtrasC)]),
        "ev2g_kernel_name": (C.c_char_p, [vp]),
        "ev2g_last_launch_specialisation": (C.c_int, [vp]),
        "ev2g_last_launch_general_reason": (C.c_char_p, [vp]),
        "ev2g_last_stats_route": (C.c_int, [vp]),
        "ev2g_last_stats_reason": (C.c_char_p, [vp]),
        "ev2g_last_launch_fast_forwarded": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "ev2g_last_launch_placement": (C.c_int, [vp, C.c_void_p, C.c_int64]),
        "ev2g_last_launch_balance": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_char_p)]),
        "ev2g_fallback_reason": (C.c_char_p, [vp]),
        "ev2g_big_kernel_reason": (C.c_char_p, [vp]),
        "ev2g_step": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        "ev2g_step_n": (C.c_int, [vp, C.c_int, C.c_int, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, C.c_int]),
        "ev2g_check_faults": (C.c_int, [vp, C.POINTER(i32)]),
        "ev2g_get_stats": (C.c_int, [vp, vp]),
        "ev2g_get_stats_reset": (C.c_int, [vp, vp, vp, C.c_int64]),
        "ev2g_get_stats_reset_f32": (C.c_int, [vp, vp, vp, C.c_int64]),
        "ev2g_reset_f32": (C.c_int, [vp, vp, C.c_int64]),
        "ev2g_collect": (C.c_int, [vp, vp, C.c_int, vp]),
        "ev2g_heuristic_create": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "ev2g_heuristic_destroy": (None, [vp, vp]),
        "ev2g_heuristic_actions": (C.c_int, [vp, vp, vp]),
        "ev2g_heuristic_run": (C.c_int, [vp, vp, C.c_int, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64]),
        "ev2g_link_create": (C.c_int, [vp, dbl, dbl, C.c_uint64, C.c_uint64, vp, vp, C.POINTER(vp)]),
        "ev2g_link_destroy": (None, [vp, vp]),
        "ev2g_link_reset_state": (C.c_int, [vp, vp]),
        "ev2g_link_actions": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp]),
        "ev2g_link_observe": (C.c_int, [vp, vp, C.c_int, vp, vp]),
        "ev2g_link_obs_f32": (vp, [vp, vp]),
        "ev2g_link_run": (C.c_int, [vp, vp, vp, C.c_int, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64]),
        "ev2g_link_rollout": (C.c_int, [vp, vp, vp, C.c_int, vp, i64, vp, i64, vp, i64]),
        "ev2g_wrap_create": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "ev2g_wrap_destroy": (None, [vp, vp]),
        "ev2g_wrap_reset_state": (C.c_int, [vp, vp]),
        "ev2g_wrap_actions": (C.c_int, [vp, vp, vp, C.c_int, vp]),
        "ev2g_wrap_run": (C.c_int, [vp, vp, C.c_int, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64]),
        "ev2g_wrap_rollout": (C.c_int, [vp, vp, vp, C.c_int, vp, i64, vp, i64, vp, i64]),
        "ev2g_grid_create": (C.c_int, [vp, C.c_int, vp, vp, dbl, dbl, C.c_int, vp, vp, C.POINTER(vp)]),
        "ev2g_grid_destroy": (None, [vp, vp]),
        "ev2g_grid_solve": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]),
        "ev2g_grid_run": (C.c_int, [vp, vp, vp, C.c_int, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, dbl, dbl]),
        "ev2g_grid_get_stats": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        "ev2g_grid_state_attach": (C.c_int, [vp, vp, vp, C.c_int]),
        "ev2g_grid_state_dim": (C.c_int, [vp, vp]),
        "ev2g_grid_observe": (C.c_int, [vp, vp, vp, vp]),
        "ev2g_grid_run_observed": (C.c_int, [vp, vp, vp, C.c_int, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, dbl, dbl, vp, i64, vp, i64]),
        "ev2g_grid_rollout": (C.c_int, [vp, vp, vp, C.c_int, vp, i64, vp, i64, vp, i64, vp, i64, dbl, dbl]),
        "ev2g_ac_create": (C.c_int, [vp] + [C.c_int] * 7 + [vp] * 13 + [C.c_float, C.c_uint64, C.POINTER(vp)]),
        "ev2g_ac_destroy": (None, [vp, vp]),
        "ev2g_ac_seed": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
        "ev2g_ac_set_log_std": (C.c_int, [vp, vp, vp]),
        "ev2g_ac_set_weights": (C.c_int, [vp, vp] + [vp] * 12),
        "ev2g_ac_forward": (C.c_int, [vp, vp, vp, C.c_int, vp, vp]),
        "ev2g_ac_act": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "ev2g_ac_collect": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(_abi.OnPolicyRowsC)]),
        "ev2g_ac_host_normal": (None, [vp, i64, C.c_uint64, C.c_uint64]),
        "ev2g_gae": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, dbl, dbl, vp, vp]),
        "ev2g_host_gae": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, dbl, dbl, vp, vp]),
        "ev2g_ppo_query": (C.c_int, [C.c_int] * 6 + [C.POINTER(_abi.PpoInfoC)]),
        "ev2g_ppo_create": (C.c_int, [vp, vp, C.POINTER(_abi.PpoConfigC), C.POINTER(vp)]),
        "ev2g_ppo_destroy": (None, [vp, vp]),
        "ev2g_ppo_set_rates": (C.c_int, [vp, vp, dbl, dbl]),
        "ev2g_ppo_grad": (C.c_int, [vp, vp] + [vp] * 6 + [C.c_int, vp]),
        "ev2g_ppo_apply": (C.c_int, [vp, vp]),
        "ev2g_ppo_minibatch": (C.c_int, [vp, vp] + [vp] * 6 + [C.c_int, vp]),
        "ev2g_ppo_get_grads": (C.c_int, [vp, vp] + [vp] * 13),
        "ev2g_ppo_sync": (C.c_int, [vp, vp]),
        "ev2g_ac_get_weights": (C.c_int, [vp, vp] + [vp] * 13),
        "ev2g_host_adam": (C.c_int, [vp, vp, vp, vp, i64, i64, dbl, dbl, dbl, dbl]),
        "ev2g_host_ppo_head": (C.c_int, [vp] * 7 + [C.c_int, C.c_int, C.POINTER(_abi.PpoConfigC), vp, vp, vp, vp]),
        "ev2g_a2c_create": (C.c_int, [vp, vp, C.POINTER(_abi.A2cConfigC), C.POINTER(vp)]),
        "ev2g_a2c_set_rate": (C.c_int, [vp, vp, dbl]),
        "ev2g_a2c_grad": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_a2c_apply": (C.c_int, [vp, vp]),
        "ev2g_a2c_update": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_host_rmsprop": (C.c_int, [vp, vp, vp, i64, dbl, dbl, dbl]),
        "ev2g_host_a2c_head": (C.c_int, [vp] * 6 + [C.c_int, C.c_int, C.POINTER(_abi.A2cConfigC), vp, vp, vp, vp]),
        "ev2g_trpo_query": (C.c_int, [C.c_int] * 6 + [C.POINTER(_abi.TrpoInfoC)]),
        "ev2g_trpo_create": (C.c_int, [vp, vp, C.POINTER(_abi.TrpoConfigC), C.POINTER(vp)]),
        "ev2g_trpo_set_rate": (C.c_int, [vp, vp, dbl]),
        "ev2g_trpo_grad": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_trpo_fvp": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, vp]),
        "ev2g_trpo_policy_step": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int]),
        "ev2g_trpo_critic_minibatch": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp]),
        "ev2g_trpo_get_report": (C.c_int, [vp, vp, C.POINTER(_abi.TrpoReportC)]),
        "ev2g_trpo_get_direction": (C.c_int, [vp, vp, vp, vp]),
        "ev2g_host_trpo_cg_step": (C.c_int, [vp, vp, vp, vp, i64, vp, C.c_int, vp]),
        "ev2g_host_trpo_rows": (C.c_int, [vp] * 7 + [C.c_int, C.c_int, C.c_int, vp, vp]),
        "ev2g_td3_default_config": (C.c_int, [C.c_int, C.POINTER(_abi.Td3ConfigC)]),
        "ev2g_td3_create": (C.c_int, [vp, vp, C.POINTER(_abi.Td3ConfigC)] + [C.c_int] * 4 + [vp, vp, C.c_uint64, C.POINTER(vp)]),
        "ev2g_td3_destroy": (None, [vp, vp]),
        "ev2g_td3_update": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_td3_critic_grad": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_td3_actor_grad": (C.c_int, [vp, vp, vp, C.c_int, vp]),
        "ev2g_td3_apply": (C.c_int, [vp, vp]),
        "ev2g_td3_get_grads": (C.c_int, [vp, vp, vp]),
        "ev2g_td3_get_weights": (C.c_int, [vp, vp, C.c_int, vp]),
        "ev2g_td3_get_y": (C.c_int, [vp, vp, vp, C.c_int]),
        "ev2g_td3_set_rate": (C.c_int, [vp, vp, dbl]),
        "ev2g_td3_seed": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
        "ev2g_td3_counters": (C.c_int, [vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_uint64)]),
        "ev2g_replay_sample": (C.c_int, [vp, C.POINTER(_abi.ReplayRingC), C.c_int, C.c_uint64, C.c_uint64] + [vp] * 6),
        "ev2g_host_replay_indices": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64]),
        "ev2g_host_td3_target": (C.c_int, [vp] * 4 + [C.c_int] * 3 + [dbl] * 3 + [C.c_uint64, C.c_uint64, vp, vp]),
        "ev2g_host_polyak": (C.c_int, [vp, vp, i64, dbl]),
        "ev2g_sac_default_config": (C.c_int, [C.POINTER(_abi.SacConfigC)]),
        "ev2g_sac_create": (C.c_int, [vp, C.POINTER(_abi.SacConfigC)] + [C.c_int] * 4 + [C.c_float, vp, vp, C.c_uint64, C.POINTER(vp)]),
        "ev2g_sac_destroy": (None, [vp, vp]),
        "ev2g_sac_update": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_sac_critic_grad": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_sac_actor_grad": (C.c_int, [vp, vp, vp, C.c_int, vp]),
        "ev2g_sac_apply": (C.c_int, [vp, vp]),
        "ev2g_sac_act": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "ev2g_sac_collect": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
        "ev2g_sac_get_grads": (C.c_int, [vp, vp, vp, vp]),
        "ev2g_sac_get_weights": (C.c_int, [vp, vp, C.c_int, vp]),
        "ev2g_sac_get_y": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "ev2g_sac_get_log_pi": (C.c_int, [vp, vp, vp, C.c_int]),
        "ev2g_sac_get_ent_coef": (C.c_int, [vp, vp, vp]),
        "ev2g_sac_set_rate": (C.c_int, [vp, vp, dbl]),
        "ev2g_sac_seed": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
        "ev2g_sac_act_seed": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
        "ev2g_sac_counters": (C.c_int, [vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "ev2g_host_sac_head": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_float, vp, vp, vp]),
        "ev2g_host_sac_head_back": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, vp, vp]),
        "ev2g_host_sac_y": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, dbl, C.c_float, vp]),
        "ev2g_tqc_default_config": (C.c_int, [C.POINTER(_abi.TqcConfigC)]),
        "ev2g_tqc_create": (C.c_int, [vp, C.POINTER(_abi.TqcConfigC)] + [C.c_int] * 4 + [C.c_float, vp, vp, C.c_uint64, C.POINTER(vp)]),
        "ev2g_tqc_destroy": (None, [vp, vp]),
        "ev2g_tqc_update": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_tqc_critic_grad": (C.c_int, [vp, vp] + [vp] * 5 + [C.c_int, vp]),
        "ev2g_tqc_actor_grad": (C.c_int, [vp, vp, vp, C.c_int, vp]),
        "ev2g_tqc_apply": (C.c_int, [vp, vp]),
        "ev2g_tqc_act": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "ev2g_tqc_collect": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
        "ev2g_tqc_get_grads": (C.c_int, [vp, vp, vp, vp]),
        "ev2g_tqc_get_weights": (C.c_int, [vp, vp, C.c_int, vp]),
        "ev2g_tqc_get_z": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "ev2g_tqc_get_log_pi": (C.c_int, [vp, vp, vp, C.c_int]),
        "ev2g_tqc_get_ent_coef": (C.c_int, [vp, vp, vp]),
        "ev2g_tqc_set_rate": (C.c_int, [vp, vp, dbl]),
        "ev2g_tqc_seed": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
        "ev2g_tqc_act_seed": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
        "ev2g_tqc_counters": (C.c_int, [vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "ev2g_tqc_truncate": (C.c_int, [vp] * 5 + [C.c_int] * 4 + [dbl, vp, vp]),
        "ev2g_host_tqc_target": (C.c_int, [vp] * 4 + [C.c_int] * 4 + [dbl, C.c_float, vp]),
        "ev2g_host_tqc_critic_head": (C.c_int, [vp, vp] + [C.c_int] * 4 + [vp, vp]),
        "ev2g_ars_default_config": (C.c_int, [C.POINTER(_abi.ArsConfigC)]),
        "ev2g_ars_query": (C.c_int, [C.POINTER(_abi.ArsConfigC)] + [C.c_int] * 5 + [C.POINTER(_abi.ArsInfoC)]),
        "ev2g_ars_create": (C.c_int, [vp, C.POINTER(_abi.ArsConfigC)] + [C.c_int] * 5 + [C.c_float, vp, C.c_uint64, C.POINTER(vp)]),
        "ev2g_ars_destroy": (None, [vp, vp]),
        "ev2g_ars_perturb": (C.c_int, [vp, vp]),
        "ev2g_ars_act": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp]),
        "ev2g_ars_obs_f32": (vp, [vp, vp]),
        "ev2g_ars_actions_f32": (vp, [vp, vp]),
        "ev2g_ars_rollout": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, i64]),
        "ev2g_ars_update": (C.c_int, [vp, vp]),
        "ev2g_ars_get_report": (C.c_int, [vp, vp, C.POINTER(_abi.ArsReportC), vp, vp]),
        "ev2g_ars_get_weights": (C.c_int, [vp, vp, vp]),
        "ev2g_ars_set_weights": (C.c_int, [vp, vp, vp]),
        "ev2g_ars_get_candidate": (C.c_int, [vp, vp, C.c_int, vp]),
        "ev2g_ars_get_deltas": (C.c_int, [vp, vp, vp]),
        "ev2g_ars_get_env_returns": (C.c_int, [vp, vp, vp, C.c_int]),
        "ev2g_ars_set_returns": (C.c_int, [vp, vp, vp]),
        "ev2g_ars_set_rates": (C.c_int, [vp, vp, dbl, dbl]),
        "ev2g_ars_seed": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
        "ev2g_ars_counters": (C.c_int, [vp, vp, C.POINTER(C.c_uint64), C.POINTER(i64), C.POINTER(i64)]),
        "ev2g_host_ars_perturb": (C.c_int, [vp, C.c_int, C.c_int, dbl, C.c_uint64, C.c_uint64, vp, vp]),
        "ev2g_host_ars_returns": (C.c_int, [vp, vp, C.c_int, i64, C.c_int, C.c_int, dbl, i64, vp]),
        "ev2g_host_ars_update": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, dbl, vp, C.POINTER(_abi.ArsReportC)]),
        "ev2g_stat_name": (C.c_char_p, [C.c_int]),
        "ev2g_peek": (C.c_int, [vp, C.c_int, C.POINTER(_abi.EnvViewC)]),
        "ev2g_malloc": (vp, [vp, C.c_size_t]),
        "ev2g_free": (None, [vp, vp]),
        "ev2g_memcpy_h2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "ev2g_memcpy_d2h": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "ev2g_host_malloc": (vp, [vp, C.c_size_t]),
        "ev2g_host_free": (None, [vp, vp]),
        "ev2g_synchronize": (C.c_int, [vp]),
        "ev2g_fill_uniform": (C.c_int, [vp, vp, i64, C.c_uint64, dbl, dbl]),
        "ev2g_host_uniform": (None, [vp, i64, C.c_uint64, dbl, dbl]),
        "ev2g_last_step_n_kernel_ms": (dbl, [vp]),
        "ev2g_mlp_create": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, C.POINTER(vp)]),
        "ev2g_mlp_create_ex": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, C.c_int, C.POINTER(vp)]),
        "ev2g_mlp_destroy": (None, [vp, vp]),
        "ev2g_mlp_forward": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "ev2g_mlp_kernel_name": (C.c_char_p, [vp]),
        "ev2g_rollout": (C.c_int, [vp, vp, C.c_int, vp, i64, vp, i64, vp, i64, C.c_int]),
        "ev2g_rollout_graph_launches": (C.c_longlong, [vp]),
        "ev2g_comm_get_unique_id": (C.c_int, [vp]),
        "ev2g_comm_init": (C.c_int, [vp, vp, C.c_int, C.c_int]),
        "ev2g_comm_destroy": (None, [vp]),
        "ev2g_step_n_kernel_ms_back": (dbl, [vp, C.c_int]),
        "ev2g_last_launch_timing": (C.c_char_p, [vp]),
        "ev2g_comm_world_size": (C.c_int, [vp]),
        "ev2g_comm_gathers": (C.c_longlong, [vp]),
        "ev2g_gather_stats": (C.c_int, [vp, vp]),
        "ev2g_pool_refill": (C.c_int, [vp, C.POINTER(_abi.GenConfigC), C.c_uint64, i64, i32, i32]),
        "ev2g_pool_refill_overflows": (C.c_longlong, [vp]),
        "ev2g_pool_session_capacity": (C.c_int, [vp]),
        "ev2g_gen_default_config": (C.c_int, [C.c_int, C.POINTER(_abi.GenConfigC)]),
        "ev2g_generate": (C.c_int, [C.POINTER(_abi.GenConfigC), i32, C.c_uint64, i32, C.POINTER(vp)]),
        "ev2g_gen_batch": (C.POINTER(_abi.ScenarioBatchC), [vp]),
        "ev2g_gen_free": (None, [vp]),
        "ev2g_gen_table": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(L, name)  # AttributeError here = the .so does not export what include/ev2g.h declares
        fn.restype = res
        fn.argtypes = args
    if L.ev2g_abi_version() != _abi.ABI_VERSION:
        raise EngineError(-1, "libev2g_hip.so ABI version mismatch")
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "ev2g_abi_version", "ev2g_create", "ev2g_destroy", "ev2g_last_error", "ev2g_load_scenarios", "ev2g_n_envs",
    "ev2g_n_scenarios", "ev2g_n_ports", "ev2g_obs_dim", "ev2g_n_steps", "ev2g_current_step", "ev2g_reset", "ev2g_reset_ex",
    "ev2g_scenario_offset", "ev2g_set_step_extras", "ev2g_kernel_name", "ev2g_last_launch_specialisation", "ev2g_last_launch_general_reason", "ev2g_last_stats_route", "ev2g_last_stats_reason", "ev2g_last_launch_fast_forwarded", "ev2g_last_launch_placement", "ev2g_last_launch_balance", "ev2g_fallback_reason", "ev2g_big_kernel_reason", "ev2g_step", "ev2g_step_n",
    "ev2g_check_faults", "ev2g_get_stats", "ev2g_get_stats_reset", "ev2g_get_stats_reset_f32", "ev2g_reset_f32", "ev2g_collect", "ev2g_stat_name", "ev2g_peek", "ev2g_malloc", "ev2g_free",
    "ev2g_memcpy_h2d", "ev2g_memcpy_d2h", "ev2g_host_malloc", "ev2g_host_free", "ev2g_synchronize", "ev2g_fill_uniform", "ev2g_host_uniform",
    "ev2g_last_step_n_kernel_ms", "ev2g_step_n_kernel_ms_back", "ev2g_last_launch_timing", "ev2g_mlp_create", "ev2g_mlp_create_ex", "ev2g_mlp_destroy", "ev2g_mlp_forward", "ev2g_mlp_kernel_name", "ev2g_rollout",
    "ev2g_rollout_graph_launches", "ev2g_comm_get_unique_id", "ev2g_comm_init", "ev2g_comm_destroy", "ev2g_comm_world_size", "ev2g_comm_gathers", "ev2g_gather_stats",
    "ev2g_pool_refill", "ev2g_pool_refill_overflows", "ev2g_pool_session_capacity", "ev2g_gen_default_config", "ev2g_generate", "ev2g_gen_batch", "ev2g_gen_free", "ev2g_gen_table",
    "ev2g_heuristic_create", "ev2g_heuristic_destroy", "ev2g_heuristic_actions", "ev2g_heuristic_run",
    "ev2g_link_create", "ev2g_link_destroy", "ev2g_link_reset_state", "ev2g_link_actions", "ev2g_link_observe", "ev2g_link_obs_f32",
    "ev2g_link_run", "ev2g_link_rollout",
    "ev2g_grid_create", "ev2g_grid_destroy", "ev2g_grid_solve", "ev2g_grid_run",
    "ev2g_grid_state_attach", "ev2g_grid_state_dim", "ev2g_grid_observe", "ev2g_grid_run_observed", "ev2g_grid_rollout", "ev2g_grid_get_stats",
    "ev2g_wrap_create", "ev2g_wrap_destroy", "ev2g_wrap_reset_state", "ev2g_wrap_actions", "ev2g_wrap_run", "ev2g_wrap_rollout",
    "ev2g_ac_create", "ev2g_ac_destroy", "ev2g_ac_seed", "ev2g_ac_set_log_std", "ev2g_ac_set_weights", "ev2g_ac_forward", "ev2g_ac_act",
    "ev2g_ac_collect", "ev2g_ac_host_normal", "ev2g_gae", "ev2g_host_gae",
    "ev2g_ppo_query", "ev2g_ppo_create", "ev2g_ppo_destroy", "ev2g_ppo_set_rates", "ev2g_ppo_grad", "ev2g_ppo_apply", "ev2g_ppo_minibatch",
    "ev2g_ppo_get_grads", "ev2g_ppo_sync", "ev2g_ac_get_weights", "ev2g_host_adam", "ev2g_host_ppo_head",
    "ev2g_a2c_create", "ev2g_a2c_set_rate", "ev2g_a2c_grad", "ev2g_a2c_apply", "ev2g_a2c_update", "ev2g_host_rmsprop", "ev2g_host_a2c_head",
    "ev2g_trpo_query", "ev2g_trpo_create", "ev2g_trpo_set_rate", "ev2g_trpo_grad", "ev2g_trpo_fvp", "ev2g_trpo_policy_step", "ev2g_trpo_critic_minibatch",
    "ev2g_trpo_get_report", "ev2g_trpo_get_direction", "ev2g_host_trpo_cg_step", "ev2g_host_trpo_rows",
    "ev2g_td3_default_config", "ev2g_td3_create", "ev2g_td3_destroy", "ev2g_td3_update", "ev2g_td3_critic_grad", "ev2g_td3_actor_grad", "ev2g_td3_apply",
    "ev2g_td3_get_grads", "ev2g_td3_get_weights", "ev2g_td3_get_y", "ev2g_td3_set_rate", "ev2g_td3_seed", "ev2g_td3_counters", "ev2g_replay_sample",
    "ev2g_host_replay_indices", "ev2g_host_td3_target", "ev2g_host_polyak",
    "ev2g_sac_default_config", "ev2g_sac_create", "ev2g_sac_destroy", "ev2g_sac_update", "ev2g_sac_critic_grad", "ev2g_sac_actor_grad", "ev2g_sac_apply",
    "ev2g_sac_act", "ev2g_sac_collect", "ev2g_sac_get_grads", "ev2g_sac_get_weights", "ev2g_sac_get_y", "ev2g_sac_get_log_pi", "ev2g_sac_get_ent_coef",
    "ev2g_sac_set_rate", "ev2g_sac_seed", "ev2g_sac_act_seed", "ev2g_sac_counters", "ev2g_host_sac_head", "ev2g_host_sac_head_back", "ev2g_host_sac_y",
    "ev2g_tqc_default_config", "ev2g_tqc_create", "ev2g_tqc_destroy", "ev2g_tqc_update", "ev2g_tqc_critic_grad", "ev2g_tqc_actor_grad", "ev2g_tqc_apply",
    "ev2g_tqc_act", "ev2g_tqc_collect", "ev2g_tqc_get_grads", "ev2g_tqc_get_weights", "ev2g_tqc_get_z", "ev2g_tqc_get_log_pi", "ev2g_tqc_get_ent_coef",
    "ev2g_tqc_set_rate", "ev2g_tqc_seed", "ev2g_tqc_act_seed", "ev2g_tqc_counters", "ev2g_tqc_truncate", "ev2g_host_tqc_target", "ev2g_host_tqc_critic_head",
    "ev2g_ars_default_config", "ev2g_ars_query", "ev2g_ars_create", "ev2g_ars_destroy", "ev2g_ars_perturb", "ev2g_ars_act", "ev2g_ars_obs_f32",
    "ev2g_ars_actions_f32", "ev2g_ars_rollout", "ev2g_ars_update", "ev2g_ars_get_report", "ev2g_ars_get_weights", "ev2g_ars_set_weights",
    "ev2g_ars_get_candidate", "ev2g_ars_get_deltas", "ev2g_ars_get_env_returns", "ev2g_ars_set_returns", "ev2g_ars_set_rates", "ev2g_ars_seed",
    "ev2g_ars_counters", "ev2g_host_ars_perturb", "ev2g_host_ars_returns", "ev2g_host_ars_update"]


def _ptr(x):
    """Device address of a DeviceBuffer / torch tensor / raw int (None -> NULL)."""
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    return int(x)


class DeviceBuffer:
    """A hipMalloc'd array owned by an engine handle (for hosts that do not use torch)."""

    def __init__(self, engine: "Engine", shape, dtype):
        self.engine = engine
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = engine._lib.ev2g_malloc(engine._h, self.nbytes)
        if not self.ptr:
            raise EngineError(-2, engine.last_error())

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, self.dtype)
        assert arr.nbytes == self.nbytes, (arr.shape, self.shape)
        self.engine._check(self.engine._lib.ev2g_memcpy_h2d(self.engine._h, self.ptr, arr.ctypes.data, self.nbytes))
        return self

    def to_host(self, out=None):
        """Copy to the host: into a new array, or into `out` (same shape / dtype, C-contiguous) so that views of it stay valid."""
        if out is None:
            out = np.empty(self.shape, self.dtype)
        else:
            assert out.dtype == self.dtype and out.nbytes == self.nbytes and out.flags.c_contiguous
        self.engine._check(self.engine._lib.ev2g_memcpy_d2h(self.engine._h, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def at(self, index_elems: int):
        return self.ptr + int(index_elems) * self.dtype.itemsize

    def free(self):
        if self.ptr and self.engine._h:
            self.engine._lib.ev2g_free(self.engine._h, self.ptr)
        self.ptr = None


class Engine:
    """One handle = one GPU = one HIP stream; E envs resident in HBM."""

    def __init__(self, batch: ScenarioBatch, reward_kind: int, state_kind: int, device: int = 0, flags: int = 0,
                 stream: Optional[int] = None, cost_kind: int = 0, n_active_envs: int = 0):
        """`batch` is the resident scenario pool (M scenarios); `n_active_envs` (default: all of them) envs are stepped
        per call, each reset choosing which window of the pool they run (`reset(offset=...)`)."""
        self._lib = load_library()
        self._h = None
        self._spec_checks_left = 4   # launches still examined by _warn_if_general
        cfg = _abi.ConfigC(int(device), int(reward_kind), int(state_kind), int(flags), stream, int(cost_kind), int(n_active_envs))
        h = C.c_void_p()
        rc = self._lib.ev2g_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise EngineError(rc, (self._lib.ev2g_last_error(None) or b"").decode())
        self._h = h
        self.reward_kind, self.state_kind, self.flags, self.device = reward_kind, state_kind, flags, device
        self.load(batch)

    # ---- scenario ----------------------------------------------------------------------------
    def load(self, batch: ScenarioBatch):
        cb = batch.to_c()
        self._check(self._lib.ev2g_load_scenarios(self._h, C.byref(cb)))
        self.batch = batch
        self.E = self._lib.ev2g_n_envs(self._h)
        self.M = self._lib.ev2g_n_scenarios(self._h)
        self.P = self._lib.ev2g_n_ports(self._h)
        self.D = self._lib.ev2g_obs_dim(self._h)
        self.T = self._lib.ev2g_n_steps(self._h)
        self.C, self.R = batch.n_chargers, batch.n_transformers
        why = self.fallback_reason
        if why and self.P <= 64:   # a shape of the common size that did not get the fast-path kernel: say so, once per cause
            import warnings
            warnings.warn(f"ev2gym_amd: step kernel {self.kernel_name} selected instead of the fast path ({why})", stacklevel=2)

    @property
    def kernel_name(self) -> str:
        """The step kernel ev2g_load_scenarios selected for the loaded shape (routing is never silent)."""
        return (self._lib.ev2g_kernel_name(self._h) or b"").decode()

    @property
    def last_launch_specialisation(self) -> int:
        """0 general / 1 full / 2 full+wide instantiation of the fast-path kernel used by the last launch (-1: none, or another kernel)."""
        return int(self._lib.ev2g_last_launch_specialisation(self._h))

    @property
    def last_stats_route(self) -> int:
        """1: the last stats() / stats_reset() copied the statistics the episode's closing step launch computed; 0: the statistics kernel
        computed them (last_stats_reason says why); -1: no such call yet."""
        return int(self._lib.ev2g_last_stats_route(self._h))

    @property
    def last_stats_reason(self) -> str:
        return (self._lib.ev2g_last_stats_reason(self._h) or b"").decode()

    @property
    def last_launch_fast_forwarded(self):
        """(workgroup-steps, stretches) of EV-free steps the last step launch fast-forwarded instead of stepping; (0, 0) after a launch that is not
        eligible or with EV2G_NO_FAST_FORWARD=1 at load time (include/ev2g.h).  Synchronises the stream."""
        n, m = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.ev2g_last_launch_fast_forwarded(self._h, C.byref(n), C.byref(m)))
        return int(n.value), int(m.value)

    @property
    def last_launch_balance(self):
        """(balanced, moved, reason): whether the last step launch had a CU-balance map (include/ev2g.h: a fast-forwarding launch from step 0), how many
        workgroups stepped another env group than without one, and -- when it had none -- why."""
        n, why = C.c_int64(0), C.c_char_p()
        on = self._lib.ev2g_last_launch_balance(self._h, C.byref(n), C.byref(why))
        return bool(on), int(n.value), (why.value or b"").decode()

    @property
    def last_launch_timing(self) -> str:
        """How the last timed call was measured (include/ev2g.h): "stamps" -- the kernel's own clock readings, a persistent step_n that is one launch of
        the fast-path kernel --, "events" -- a HIP-event pair around the call's launches --, or "" where last_step_n_kernel_ms reads -1."""
        return (self._lib.ev2g_last_launch_timing(self._h) or b"").decode()

    def last_launch_placement(self):
        """Development (EV2G_PLACEMENT=1 at load time, include/ev2g.h): [n_workgroups, 2] uint32 -- hardware ids and arrival rank on its CU of every workgroup
        of the last fast-forwarding launch; None when nothing was recorded.  Synchronises the stream."""
        out = np.zeros((2 * ((self.E + 3) // 4 + 1),), np.uint32)
        n = int(self._lib.ev2g_last_launch_placement(self._h, out.ctypes.data, out.size))
        if n < 0:
            self._check(n)
        return out[:2 * n].reshape(n, 2) if n else None

    @property
    def fallback_reason(self) -> str:
        return (self._lib.ev2g_fallback_reason(self._h) or b"").decode()

    @property
    def big_kernel_reason(self) -> str:
        """Why a big env (512 < ports <= 1024) does NOT get `ev2g_step_big` for its specialised launches ("" when it does / not a big env)."""
        return (self._lib.ev2g_big_kernel_reason(self._h) or b"").decode()

    @property
    def scenario_offset(self) -> int:
        return int(self._lib.ev2g_scenario_offset(self._h))

    def set_extras(self, cost=None, cost_stride=0, obs_f32=None, obs_f32_stride=0, actions_f32=None):
        """Optional sticky step outputs / inputs (include/ev2g.h ev2g_step_extras); all None clears them."""
        self._extras_keep = (cost, obs_f32, actions_f32)   # keep the buffers alive
        x = _abi.StepExtrasC(_ptr(cost), int(cost_stride), _ptr(obs_f32), int(obs_f32_stride), _ptr(actions_f32))
        self._check(self._lib.ev2g_set_step_extras(self._h, C.byref(x)))

    # ---- plumbing ------------------------------------------------------------------------------
    def last_error(self) -> str:
        return (self._lib.ev2g_last_error(self._h) or b"").decode()

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.last_error())

    def empty(self, shape, dtype=np.float64) -> DeviceBuffer:
        return DeviceBuffer(self, shape, dtype)

    def pinned(self, shape, dtype=np.float64) -> np.ndarray:
        """A numpy array over page-locked host memory (ev2g_host_malloc): the destination / source of per-step copies (the SB3 VecEnv
        hand-over).  The memory belongs to the handle: the array must not be used after `close()`."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = self._lib.ev2g_host_malloc(self._h, max(n, 1))
        if not p:
            raise EngineError("ev2g_host_malloc failed")
        buf = (C.c_char * max(n, 1)).from_address(p)
        return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def memcpy_d2h(self, host_array: np.ndarray, dev_ptr, nbytes: int):
        """One device -> host copy of `nbytes` from a raw device address into a (pinned or ordinary) C-contiguous host array."""
        assert host_array.flags.c_contiguous and host_array.nbytes >= nbytes
        self._check(self._lib.ev2g_memcpy_d2h(self._h, host_array.ctypes.data, _ptr(dev_ptr), int(nbytes)))

    def synchronize(self):
        self._check(self._lib.ev2g_synchronize(self._h))

    @property
    def current_step(self) -> int:
        return self._lib.ev2g_current_step(self._h)

    # ---- hot path ------------------------------------------------------------------------------
    def reset(self, obs=None, offset: Optional[int] = None):
        """Re-arm every env; `offset` first draws the scenarios of the coming episode: env e runs scenario
        (e + offset) mod M of the resident pool (None: the same scenarios as before)."""
        if offset is None:
            self._check(self._lib.ev2g_reset(self._h, _ptr(obs)))
        else:
            self._check(self._lib.ev2g_reset_ex(self._h, _ptr(obs), int(offset)))

    def _warn_if_general(self):
        """The fast path has a specialised instantiation (~20 % faster) that a launch gets only when it passes every output with step
        stride 0 and no extras (include/ev2g.h).  Falling off it is legal but silent: the first launches of an engine are checked and the
        caller is told, once, which argument did it (like the kernel-routing warning at load)."""
        if self._spec_checks_left <= 0:
            return
        self._spec_checks_left -= 1
        if self._lib.ev2g_last_launch_specialisation(self._h) == 0:
            why = (self._lib.ev2g_last_launch_general_reason(self._h) or b"").decode()
            # only for arguments a caller would change to get the fast instantiation back (a missing output, mismatched buffers, strides
            # a narrow env cannot specialise on): modes that are legitimate API use -- auto_reset (the gym / vec-env default), a registered
            # cost buffer, charger histories, a run-time reward -- are not performance mistakes and stay silent
            quiet = ("EV2G_NO_FULL", "auto_reset", "a cost buffer", "EV2G_FLAG_LOG_CS_HISTORY", "the reward function")
            if why and not why.startswith(quiet):
                self._spec_checks_left = 0
                warnings.warn(f"ev2gym_amd: this launch ran the GENERAL instantiation of {self.kernel_name} (slower than the full one): {why}", stacklevel=3)

    def step(self, actions, obs=None, reward=None, done=None, mask=None):
        self._check(self._lib.ev2g_step(self._h, _ptr(actions), _ptr(obs), _ptr(reward), _ptr(done), _ptr(mask)))
        if self._spec_checks_left > 0:
            self._warn_if_general()

    def step_n(self, k, actions, a_stride, obs=None, o_stride=0, reward=None, r_stride=0, done=None, d_stride=0,
               mask=None, m_stride=0, auto_reset=True, persistent=False):
        rc = self._lib.ev2g_step_n(self._h, int(k), 1 if persistent else 0, _ptr(actions), int(a_stride), _ptr(obs),
                                   int(o_stride), _ptr(reward), int(r_stride), _ptr(done), int(d_stride), _ptr(mask),
                                   int(m_stride), int(auto_reset))   # 0 / AUTO_RESET_SAME (True) / AUTO_RESET_NEXT
        self._check(rc)
        if self._spec_checks_left > 0:
            self._warn_if_general()

    # ---- policy in the loop ----------------------------------------------------------------------
    def mlp_create(self, W1, b1, W2, b2, W3, b3, out_lo=-1.0, precision="bf16"):
        """Three-layer actor (torch.nn.Linear layout: W[out,in], b[out]; host float32 arrays) evaluated by one fused kernel.
        precision: "bf16" (bf16 operands, fp32 accumulation: fastest), "fp32" (float32 weights as two bf16 terms, five products per
        k-step: within 1e-5 of a float64 forward -- what a float32-trained policy, e.g. SB3's, computes -- at twice the bf16 time) or
        "fp32x3" (three terms, all 24 bits: 1e-7 level, 2.6x the bf16 time); see include/ev2g.h."""
        arrs = [np.ascontiguousarray(a, np.float32) for a in (W1, b1, W2, b2, W3, b3)]
        h1, d_in = arrs[0].shape
        h2, d_out = arrs[2].shape[0], arrs[4].shape[0]
        assert arrs[2].shape == (h2, h1) and arrs[4].shape == (d_out, h2) and arrs[1].shape == (h1,) and arrs[3].shape == (h2,) and arrs[5].shape == (d_out,)
        m = C.c_void_p()
        prec = {"bf16": 0, "fp32": 1, "f32": 1, "fp32x3": 2, "f32x3": 2}[precision]
        self._check(self._lib.ev2g_mlp_create_ex(self._h, d_in, h1, h2, d_out, *[a.ctypes.data for a in arrs], float(out_lo), prec, C.byref(m)))
        return m

    def mlp_destroy(self, m):
        if self._h:
            self._lib.ev2g_mlp_destroy(self._h, m)

    def mlp_forward(self, m, x, y, n_rows):
        self._check(self._lib.ev2g_mlp_forward(self._h, m, _ptr(x), _ptr(y), int(n_rows)))

    def mlp_kernel_name(self, m) -> str:
        """The actor kernel instantiation the policy got, e.g. "ev2g_mlp3_s16<6,25,19,4,1,8>; from 4097 rows ev2g_mlp3_s16<6,25,19,4,1,4,2>"
        (include/ev2g.h: ev2g_mlp_kernel_name)."""
        return (self._lib.ev2g_mlp_kernel_name(m) or b"").decode()

    def rollout(self, m, k, reward=None, r_stride=0, done=None, d_stride=0, mask=None, m_stride=0, auto_reset=0):
        """k x (actor forward on the registered float32 observation -> float32 actions -> env step), one C call."""
        self._check(self._lib.ev2g_rollout(self._h, m, int(k), _ptr(reward), int(r_stride), _ptr(done), int(d_stride), _ptr(mask),
                                           int(m_stride), int(auto_reset)))

    @property
    def rollout_graph_launches(self) -> int:
        return int(self._lib.ev2g_rollout_graph_launches(self._h))

    def last_step_n_kernel_ms(self) -> float:
        return float(self._lib.ev2g_last_step_n_kernel_ms(self._h))

    def step_n_kernel_ms_back(self, back: int) -> float:
        """HIP-event duration of the timed call `back` calls before the last one (the handle keeps 32): queue launches, read them afterwards."""
        return float(self._lib.ev2g_step_n_kernel_ms_back(self._h, int(back)))

    def check_faults(self):
        bad = C.c_int32(-1)
        rc = self._lib.ev2g_check_faults(self._h, C.byref(bad))
        if rc != 0:
            raise EngineError(rc, f"env {bad.value}: " + self.last_error())

    def fill_uniform(self, dst, n, seed, lo, hi):
        self._check(self._lib.ev2g_fill_uniform(self._h, _ptr(dst), int(n), int(seed), float(lo), float(hi)))

    # ---- the env-reading heuristic agents on the device (include/ev2g.h: ev2g_heuristic_*) ----------------------------------------
    def heuristic_create(self, name):
        """A device-resident agent of the reference's heuristic `name` (a key of _abi.AGENT_KINDS, or the kind number), bound to this
        engine's envs and ports; freed by heuristic_destroy or with the engine.  The two RoundRobin_GF agents need one port per charger."""
        kind = _abi.AGENT_KINDS[name] if isinstance(name, str) else int(name)
        a = C.c_void_p()
        self._check(self._lib.ev2g_heuristic_create(self._h, kind, C.byref(a)))
        return a

    def heuristic_destroy(self, a):
        if self._h and a:
            self._lib.ev2g_heuristic_destroy(self._h, a)

    def heuristic_actions(self, a, out):
        """The agent's float64 actions [E, P] for the current step into the device array `out` (DeviceBuffer or torch tensor); no step."""
        self._check(self._lib.ev2g_heuristic_actions(self._h, a, _ptr(out)))

    def heuristic_run(self, a, k, actions=None, a_stride=0, obs=None, o_stride=0, reward=None, r_stride=0, done=None, d_stride=0,
                      mask=None, m_stride=0):
        """k x (agent -> one step) inside one episode, outputs as in step_n; timed like step_n (last_step_n_kernel_ms)."""
        self._check(self._lib.ev2g_heuristic_run(self._h, a, int(k), _ptr(actions), int(a_stride), _ptr(obs), int(o_stride), _ptr(reward),
                                                 int(r_stride), _ptr(done), int(d_stride), _ptr(mask), int(m_stride)))

    # ---- the reference's communication-fault models on the device (include/ev2g.h: ev2g_link_*) -----------------------------------
    def link_create(self, p_fail=0.0, p_delay=0.0, seed_act=0, seed_obs=0, rand_act=None, rand_obs=None):
        """A link of FailedActionCommunication (p_fail) and DelayedObservation (p_delay; PublicPST only) for this engine's envs
        (rl_agent/noise_wrappers.py), freed by link_destroy or with the engine.  rand_act / rand_obs: host matrices [E, P, T] (env e's [P, T]
        block is the reference wrapper's `random`), or None: generated from the seed, the bits of host_uniform(E * P * T, seed, 0, 1)."""
        keep = []
        for r in (rand_act, rand_obs):
            if r is not None:
                r = np.ascontiguousarray(r, np.float64)
                if r.shape != (self.E, self.P, self.T):
                    raise ValueError(f"link_create: a uniform matrix has shape {r.shape}, expected {(self.E, self.P, self.T)}")
            keep.append(r)
        l = C.c_void_p()
        self._check(self._lib.ev2g_link_create(self._h, float(p_fail), float(p_delay), int(seed_act) & (2 ** 64 - 1), int(seed_obs) & (2 ** 64 - 1),
                                               *[None if r is None else r.ctypes.data for r in keep], C.byref(l)))
        return l

    def link_destroy(self, l):
        if self._h and l:
            self._lib.ev2g_link_destroy(self._h, l)

    def link_reset_state(self, l):
        """Zero the held commands and the remembered observation columns (a freshly constructed pair of wrappers)."""
        self._check(self._lib.ev2g_link_reset_state(self._h, l))

    def link_actions(self, l, actions, out=None, t=-1, f32=False):
        """The delivered commands of step t (default: the current step) for the raw device actions [E, P] (float64, or float32 with f32=True)
        into the link and into the float64 device array `out`; no step."""
        self._check(self._lib.ev2g_link_actions(self._h, l, int(t), _ptr(actions), int(bool(f32)), _ptr(out)))

    def link_observe(self, l, obs, obs32=None, t=-1):
        """Rewrite the device observation [E, D] of step t (default: the current step; 0 = the reset observation) as DelayedObservation delivers
        it; obs32 receives the float32 copy."""
        self._check(self._lib.ev2g_link_observe(self._h, l, int(t), _ptr(obs), _ptr(obs32)))

    def link_obs_f32(self, l) -> int:
        """Device address of the link's float32 delivered row [E, D], the policy input of link_rollout."""
        p = self._lib.ev2g_link_obs_f32(self._h, l)
        if not p:
            raise EngineError(-1, self.last_error())
        return int(p)

    def link_run(self, l, k, agent=None, actions=None, a_stride=0, obs=None, o_stride=0, reward=None, r_stride=0, done=None, d_stride=0,
                 mask=None, m_stride=0):
        """k x ([agent ->] held commands -> one step -> delayed observation) inside one episode; outputs as in step_n, timed like it."""
        self._check(self._lib.ev2g_link_run(self._h, l, agent, int(k), _ptr(actions), int(a_stride), _ptr(obs), int(o_stride), _ptr(reward),
                                            int(r_stride), _ptr(done), int(d_stride), _ptr(mask), int(m_stride)))

    def link_rollout(self, l, m, k, reward=None, r_stride=0, done=None, d_stride=0, mask=None, m_stride=0):
        """k x (actor on the link's float32 delivered row -> held commands -> one step -> delayed observation), unfused, inside one episode."""
        self._check(self._lib.ev2g_link_rollout(self._h, l, m, int(k), _ptr(reward), int(r_stride), _ptr(done), int(d_stride), _ptr(mask),
                                                int(m_stride)))

    # ---- the reference's action wrappers on the device (include/ev2g.h: ev2g_wrap_*) ----------------------------------------------
    def wrap_create(self, name):
        """A device-resident action wrapper of the reference's class `name` (a key of _abi.WRAP_KINDS, or the kind number), bound to this
        engine's envs and ports; freed by wrap_destroy or with the engine.  Rescale_RepairLayer needs one port per charger."""
        kind = _abi.WRAP_KINDS[name] if isinstance(name, str) else int(name)
        w = C.c_void_p()
        self._check(self._lib.ev2g_wrap_create(self._h, kind, C.byref(w)))
        return w

    def wrap_destroy(self, w):
        if self._h and w:
            self._lib.ev2g_wrap_destroy(self._h, w)

    def wrap_reset_state(self, w):
        """Empty the repair layer's queue (a freshly constructed wrapper); nothing to do for the discretisers."""
        self._check(self._lib.ev2g_wrap_reset_state(self._h, w))

    def wrap_actions(self, w, actions, out, f32=False):
        """The wrapper's action() at the current step for the raw device actions [E, P] (float64, or float32 with f32=True) into the float64
        device array `out`, which may be a float64 `actions`; no step."""
        self._check(self._lib.ev2g_wrap_actions(self._h, w, _ptr(actions), int(bool(f32)), _ptr(out)))

    def wrap_run(self, w, k, actions, a_stride=0, wrapped=None, w_stride=0, obs=None, o_stride=0, reward=None, r_stride=0, done=None,
                 d_stride=0, mask=None, m_stride=0):
        """k x (wrapper -> one step) inside one episode on the raw actions [k, E, P]; the wrapped actions go to `wrapped`; outputs as in
        step_n, timed like it."""
        self._check(self._lib.ev2g_wrap_run(self._h, w, int(k), _ptr(actions), int(a_stride), _ptr(wrapped), int(w_stride), _ptr(obs),
                                            int(o_stride), _ptr(reward), int(r_stride), _ptr(done), int(d_stride), _ptr(mask), int(m_stride)))

    def wrap_rollout(self, w, m, k, reward=None, r_stride=0, done=None, d_stride=0, mask=None, m_stride=0):
        """k x (actor between the registered float32 buffers -> wrapper -> one step), unfused, inside one episode."""
        self._check(self._lib.ev2g_wrap_rollout(self._h, w, m, int(k), _ptr(reward), int(r_stride), _ptr(done), int(d_stride), _ptr(mask),
                                                int(m_stride)))

    # ---- the distribution grid's power flow on the device (include/ev2g.h: ev2g_grid_*) ------------------------------------------
    def grid_create(self, network, profiles=None, tolerance=1e-6, max_iter=100):
        """A device-resident Laurent power flow of `network` (ev2gym_amd.grid.GridNetwork, or anything with n_bus, K, L, s_base), freed by
        grid_destroy or with the engine.  profiles = (p_base, q_base), host arrays [M, T + 1, n_bus - 1] in kW (GridNetwork.base_profiles), make
        it usable by grid_run: the scenarios then need one transformer per non-slack bus.  None: the solver only (grid_solve)."""
        n = int(network.n_bus) - 1
        K = np.ascontiguousarray(network.K, np.complex128)
        L = np.ascontiguousarray(np.asarray(network.L).reshape(-1), np.complex128)
        if K.shape != (n, n) or L.shape != (n,):
            raise ValueError(f"grid_create: K {K.shape} / L {L.shape} do not fit {n + 1} buses")
        pq = [None, None]
        if profiles is not None:
            pq = [np.ascontiguousarray(x, np.float64) for x in profiles]
            want = (self.M, self.T + 1, n)
            for x in pq:
                if x.shape != want:
                    raise ValueError(f"grid_create: a base profile has shape {x.shape}, expected {want} (scenarios of the pool, steps + 1, non-slack buses)")
        g = C.c_void_p()
        self._check(self._lib.ev2g_grid_create(self._h, n + 1, K.ctypes.data, L.ctypes.data, float(network.s_base), float(tolerance), int(max_iter),
                                               *[None if x is None else x.ctypes.data for x in pq], C.byref(g)))
        return g

    def grid_destroy(self, g):
        if self._h and g:
            self._lib.ev2g_grid_destroy(self._h, g)

    def grid_solve(self, g, p_kw, q_kw, n_rows, vm=None, v_complex=None, iters=None, loss_v=None):
        """The bare batched solver on device arrays: p_kw / q_kw [n_rows, n] in kW -> vm [n_rows, n_bus], v_complex [n_rows, n, 2],
        iters [n_rows] int32, loss_v [n_rows] (each optional)."""
        self._check(self._lib.ev2g_grid_solve(self._h, g, _ptr(p_kw), _ptr(q_kw), int(n_rows), _ptr(vm), _ptr(v_complex), _ptr(iters), _ptr(loss_v)))

    def grid_run(self, g, k, agent=None, actions=None, a_stride=0, obs=None, o_stride=0, reward=None, r_stride=0, done=None, d_stride=0,
                 mask=None, m_stride=0, vm=None, v_stride=0, base_weight=0.0, voltage_weight=1000.0):
        """k x ([agent ->] one step -> power flow on that step's transformer powers) inside one episode; outputs as in step_n plus the bus
        voltages vm [k, E, n_bus]; reward = base_weight * the step's reward + voltage_weight * loss_v.  Timed like step_n."""
        self._check(self._lib.ev2g_grid_run(self._h, g, agent, int(k), _ptr(actions), int(a_stride), _ptr(obs), int(o_stride), _ptr(reward),
                                            int(r_stride), _ptr(done), int(d_stride), _ptr(mask), int(m_stride), _ptr(vm), int(v_stride),
                                            float(base_weight), float(voltage_weight)))

    def grid_state_attach(self, g, time_features):
        """Attach V2G_grid_state (rl_agent/state.py:216-278) to a grid made with profiles: time_features [T + 1, 3] (ev2gym_amd.grid.time_features;
        every scenario of the pool starts at the same date) or [M, T + 1, 3].  Returns the row width Dg."""
        tf = np.ascontiguousarray(time_features, np.float64)
        if tf.shape not in ((self.T + 1, 3), (self.M, self.T + 1, 3)):
            raise ValueError(f"grid_state_attach: time_features has shape {tf.shape}, expected {(self.T + 1, 3)} or {(self.M, self.T + 1, 3)} "
                             "(steps + 1 rows of weekday / 7, sin, cos)")
        self._check(self._lib.ev2g_grid_state_attach(self._h, g, tf.ctypes.data, int(tf.ndim == 3)))
        return self.grid_state_dim(g)

    def grid_state_dim(self, g) -> int:
        """6 + 2 (n_bus - 1) + 3 P, or -1 when no state is attached to the grid."""
        return int(self._lib.ev2g_grid_state_dim(self._h, g))

    def grid_observe(self, g, obs=None, obs32=None):
        """The V2G_grid_state rows [E, Dg] of the current step counter into the device arrays obs (float64) / obs32 (float32), and into the
        grid's own rows (what grid_rollout starts from)."""
        self._check(self._lib.ev2g_grid_observe(self._h, g, _ptr(obs), _ptr(obs32)))

    def grid_run_observed(self, g, k, agent=None, actions=None, a_stride=0, obs=None, o_stride=0, reward=None, r_stride=0, done=None, d_stride=0,
                          mask=None, m_stride=0, vm=None, v_stride=0, base_weight=0.0, voltage_weight=1000.0, gobs=None, go_stride=0,
                          gobs32=None, go32_stride=0):
        """grid_run, and after each step's power flow the V2G_grid_state rows of the next step counter into gobs [k, E, Dg] / gobs32."""
        self._check(self._lib.ev2g_grid_run_observed(self._h, g, agent, int(k), _ptr(actions), int(a_stride), _ptr(obs), int(o_stride),
                                                     _ptr(reward), int(r_stride), _ptr(done), int(d_stride), _ptr(mask), int(m_stride), _ptr(vm),
                                                     int(v_stride), float(base_weight), float(voltage_weight), _ptr(gobs), int(go_stride),
                                                     _ptr(gobs32), int(go32_stride)))

    def grid_rollout(self, g, m, k, reward=None, r_stride=0, done=None, d_stride=0, mask=None, m_stride=0, vm=None, v_stride=0,
                     base_weight=0.0, voltage_weight=1000.0):
        """k x (actor on the grid's float32 state row -> one step -> power flow -> next state row), unfused, inside one episode; grid_observe
        first.  The actor maps Dg -> P."""
        self._check(self._lib.ev2g_grid_rollout(self._h, g, m, int(k), _ptr(reward), int(r_stride), _ptr(done), int(d_stride), _ptr(mask),
                                                int(m_stride), _ptr(vm), int(v_stride), float(base_weight), float(voltage_weight)))

    def grid_get_stats(self, g) -> dict:
        """The episode's voltage statistics kept by the grid kernel, [E] host arrays: voltage_violation, voltage_violation_counter,
        voltage_violation_counter_per_step (utilities/utils.py:69-78) and total_reward, the sum of the composed rewards."""
        vv, rs = np.empty(self.E, np.float64), np.empty(self.E, np.float64)
        cnt, steps = np.empty(self.E, np.int32), np.empty(self.E, np.int32)
        self._check(self._lib.ev2g_grid_get_stats(self._h, g, vv.ctypes.data, cnt.ctypes.data, steps.ctypes.data, rs.ctypes.data))
        return dict(voltage_violation=vv, voltage_violation_counter=cnt, voltage_violation_counter_per_step=steps, total_reward=rs)

    # ---- on-policy rollouts on the device (include/ev2g.h: ev2g_ac_*, ev2g_gae) ----------------------------------------------------
    def ac_create(self, weights, log_std, activation="tanh", lo=-1.0, seed=0):
        """A device-resident Gaussian actor-critic (SB3's default ActorCriticPolicy for a Box action space), freed by ac_destroy or with the
        engine.  weights: the twelve host arrays in the order of ev2g_ac_create -- policy trunk (W1, b1, W2, b2), value trunk (W1, b1, W2,
        b2), action head (W, b), value head (W, b) -- in torch.nn.Linear layout; ev2gym_amd.onpolicy.GaussianActorCritic checks the shapes."""
        arrs = [np.ascontiguousarray(a, np.float32) for a in weights]
        assert len(arrs) == 12
        ls = np.ascontiguousarray(log_std, np.float32)
        widths = _abi.ac_widths(arrs)
        act = _abi.AC_ACTIVATIONS[activation] if isinstance(activation, str) else int(activation)
        ac = C.c_void_p()
        self._check(self._lib.ev2g_ac_create(self._h, *widths, act, *[a.ctypes.data for a in arrs], ls.ctypes.data,
                                             float(lo), int(seed) & (2 ** 64 - 1), C.byref(ac)))
        return ac

    def ac_destroy(self, ac):
        if self._h and ac:
            self._lib.ev2g_ac_destroy(self._h, ac)

    def ac_seed(self, ac, seed, first_draw=0):
        """The noise stream's seed and the launch counter the next sampling launch uses."""
        self._check(self._lib.ev2g_ac_seed(self._h, ac, int(seed) & (2 ** 64 - 1), int(first_draw)))

    def ac_set_log_std(self, ac, log_std):
        ls = np.ascontiguousarray(log_std, np.float32)
        self._check(self._lib.ev2g_ac_set_log_std(self._h, ac, ls.ctypes.data))

    def ac_set_weights(self, ac, weights):
        arrs = [np.ascontiguousarray(a, np.float32) for a in weights]
        assert len(arrs) == 12
        self._check(self._lib.ev2g_ac_set_weights(self._h, ac, *[a.ctypes.data for a in arrs]))

    def ac_forward(self, ac, obs32, n_rows, mean=None, value=None):
        """mean [n_rows, P] / value [n_rows] of the float32 device rows obs32 [n_rows, D]; nothing sampled, no counter advanced."""
        self._check(self._lib.ev2g_ac_forward(self._h, ac, _ptr(obs32), int(n_rows), _ptr(mean), _ptr(value)))

    def ac_act(self, ac, obs32, n_rows, actions=None, clipped=None, value=None, log_prob=None, deterministic=False):
        """One sampling launch on device rows, no step: the unclipped sample, clip(sample, lo, 1), the value and the log-probability."""
        self._check(self._lib.ev2g_ac_act(self._h, ac, _ptr(obs32), int(n_rows), int(bool(deterministic)), _ptr(actions), _ptr(clipped),
                                          _ptr(value), _ptr(log_prob)))

    def ac_collect(self, ac, k, obs, actions, values, log_probs, reward, done, mask, deterministic=False):
        """k x (sampling launch -> env step) inside one episode, the rows written straight into the caller's DEVICE arrays (ev2g_ac_collect):
        obs float32 [k + 1, E, D] (row 0 is the input observation), actions float32 [k, E, P] (unclipped), values / log_probs float32 [k, E],
        reward float64 [k, E], done / mask uint8."""
        rows = _abi.OnPolicyRowsC(_ptr(obs), _ptr(actions), _ptr(values), _ptr(log_probs), _ptr(reward), _ptr(done), _ptr(mask))
        self._check(self._lib.ev2g_ac_collect(self._h, ac, int(k), int(bool(deterministic)), C.byref(rows)))

    def gae(self, reward, values, episode_starts, last_values, last_dones, k, n_envs, gamma, gae_lambda, advantages, returns):
        """RolloutBuffer.compute_returns_and_advantage on device arrays (ev2g_gae): reward float64 [k, n_envs], values float32, episode_starts
        uint8, last_values float32 [n_envs], last_dones uint8 [n_envs] -> advantages / returns float32 [k, n_envs]."""
        self._check(self._lib.ev2g_gae(self._h, _ptr(reward), _ptr(values), _ptr(episode_starts), _ptr(last_values), _ptr(last_dones), int(k),
                                       int(n_envs), float(gamma), float(gae_lambda), _ptr(advantages), _ptr(returns)))

    # ---- statistics / inspection ---------------------------------------------------------------
    # ---- the PPO learner (include/ev2g.h: ev2g_ppo_*) ---------------------------------------------------------------------------------
    def ac_get_weights(self, ac, ac_shape):
        """(the twelve arrays, log_std) of a device policy as host float32 arrays (ev2g_ac_get_weights): the learner's masters when one is bound.
        ac_shape: (d_in, h1, h2, v1, v2, d_out)."""
        out = [np.empty(s, np.float32) for s in _abi.ac_param_shapes(*ac_shape)]
        self._check(self._lib.ev2g_ac_get_weights(self._h, ac, *[a.ctypes.data for a in out]))
        return out[:12], out[12]

    def ppo_create(self, ac, lr=3e-4, beta1=0.9, beta2=0.999, adam_eps=1e-5, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5,
                   normalize_advantage=True):
        """A PPO learner bound to the device policy `ac` (ev2g_ppo_create), freed by ppo_destroy, with its policy or with the engine."""
        cfg = _abi.PpoConfigC(float(lr), float(beta1), float(beta2), float(adam_eps), float(clip_range), float(vf_coef), float(ent_coef),
                              float(max_grad_norm), int(bool(normalize_advantage)))
        out = C.c_void_p()
        self._check(self._lib.ev2g_ppo_create(self._h, ac, C.byref(cfg), C.byref(out)))
        return out.value

    def ppo_destroy(self, ppo):
        if ppo and self._h:
            self._lib.ev2g_ppo_destroy(self._h, ppo)

    def ppo_set_rates(self, ppo, lr, clip_range):
        self._check(self._lib.ev2g_ppo_set_rates(self._h, ppo, float(lr), float(clip_range)))

    def _learner_rows(self, entry, learner, arrays, idx, B, stats):
        """A grad / minibatch / update entry of either kind over rows idx [B] (int32) of the DEVICE float32 `arrays`."""
        self._check(getattr(self._lib, entry)(self._h, learner, *map(_ptr, arrays), _ptr(idx), int(B), _ptr(stats)))

    def ppo_grad(self, ppo, obs, actions, old_log_prob, advantages, returns, idx, B, stats=None):
        """The gradient of the minibatch idx [B] (int32) of the DEVICE float32 arrays; stays in the learner.  stats: float32 [6] DEVICE or None."""
        self._learner_rows("ev2g_ppo_grad", ppo, (obs, actions, old_log_prob, advantages, returns), idx, B, stats)

    def ppo_apply(self, ppo):
        self._check(self._lib.ev2g_ppo_apply(self._h, ppo))

    def ppo_minibatch(self, ppo, obs, actions, old_log_prob, advantages, returns, idx, B, stats=None):
        self._learner_rows("ev2g_ppo_minibatch", ppo, (obs, actions, old_log_prob, advantages, returns), idx, B, stats)

    def ppo_get_grads(self, ppo, ac_shape):
        """The last gradient (unclipped) as thirteen host float32 arrays in SB3's layout: the twelve of ac_create's order, then log_std."""
        out = [np.empty(s, np.float32) for s in _abi.ac_param_shapes(*ac_shape)]
        self._check(self._lib.ev2g_ppo_get_grads(self._h, ppo, *[a.ctypes.data for a in out]))
        return out

    def ppo_sync(self, ppo):
        self._check(self._lib.ev2g_ppo_sync(self._h, ppo))

    # ---- the A2C learner (include/ev2g.h: ev2g_a2c_*); ppo_destroy / ppo_get_grads / ppo_sync serve it too ------------------------------
    def a2c_create(self, ac, lr=7e-4, alpha=0.99, rms_eps=1e-5, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, normalize_advantage=False,
                   use_rms_prop=True):
        """An A2C learner bound to the device policy `ac` (ev2g_a2c_create), freed by ppo_destroy, with its policy or with the engine."""
        cfg = _abi.A2cConfigC(float(lr), float(alpha), float(rms_eps), float(vf_coef), float(ent_coef), float(max_grad_norm),
                              int(bool(normalize_advantage)), int(bool(use_rms_prop)))
        out = C.c_void_p()
        self._check(self._lib.ev2g_a2c_create(self._h, ac, C.byref(cfg), C.byref(out)))
        return out.value

    def a2c_set_rate(self, learner, lr):
        self._check(self._lib.ev2g_a2c_set_rate(self._h, learner, float(lr)))

    def a2c_grad(self, learner, obs, actions, advantages, returns, idx, B, stats=None):
        """The gradient of one update over rows idx [B] (int32) of the DEVICE float32 arrays; stays in the learner.  stats: float32 [6] DEVICE or None."""
        self._learner_rows("ev2g_a2c_grad", learner, (obs, actions, advantages, returns), idx, B, stats)

    def a2c_apply(self, learner):
        self._check(self._lib.ev2g_a2c_apply(self._h, learner))

    def a2c_update(self, learner, obs, actions, advantages, returns, idx, B, stats=None):
        self._learner_rows("ev2g_a2c_update", learner, (obs, actions, advantages, returns), idx, B, stats)

    # ---- the TRPO learner (include/ev2g.h: ev2g_trpo_*); ppo_destroy / ppo_get_grads / ppo_sync serve it too -----------------------------
    def trpo_create(self, ac, lr=1e-3, target_kl=0.01, cg_damping=0.1, line_search_shrinking_factor=0.8, cg_max_steps=15, line_search_max_iter=10,
                    normalize_advantage=True):
        """A TRPO learner bound to the device policy `ac` (ev2g_trpo_create), freed by ppo_destroy, with its policy or with the engine."""
        cfg = _abi.TrpoConfigC(float(lr), float(target_kl), float(cg_damping), float(line_search_shrinking_factor), int(cg_max_steps),
                               int(line_search_max_iter), int(bool(normalize_advantage)))
        out = C.c_void_p()
        self._check(self._lib.ev2g_trpo_create(self._h, ac, C.byref(cfg), C.byref(out)))
        return out.value

    def trpo_set_rate(self, learner, lr):
        self._check(self._lib.ev2g_trpo_set_rate(self._h, learner, float(lr)))

    def trpo_grad(self, learner, obs, actions, old_log_prob, advantages, idx, B, objective=None):
        """g, J(theta0) and mu0 over rows idx [B] (int32) of the DEVICE float32 arrays; g goes into the actor's arrays of ppo_get_grads.
        objective: float64 [1] DEVICE or None."""
        self._learner_rows("ev2g_trpo_grad", learner, (obs, actions, old_log_prob, advantages), idx, B, objective)

    def trpo_fvp(self, learner, obs, idx, B, v, Hv):
        """One Fisher-vector product, damping included: v, Hv float32 [n_actor] DEVICE, flat in the actor's order."""
        self._check(self._lib.ev2g_trpo_fvp(self._h, learner, _ptr(obs), _ptr(idx), int(B), _ptr(v), _ptr(Hv)))

    def trpo_policy_step(self, learner, obs, actions, old_log_prob, advantages, idx, B):
        """The whole natural-gradient step over rows idx [B]: asynchronous (trpo_get_report or ppo_sync waits for it)."""
        self._check(self._lib.ev2g_trpo_policy_step(self._h, learner, _ptr(obs), _ptr(actions), _ptr(old_log_prob), _ptr(advantages), _ptr(idx), int(B)))

    def trpo_critic_minibatch(self, learner, obs, returns, idx, B, value_loss=None):
        """One Adam step of the value function over rows idx [B]; value_loss: float32 [1] DEVICE or None."""
        self._check(self._lib.ev2g_trpo_critic_minibatch(self._h, learner, _ptr(obs), _ptr(returns), _ptr(idx), int(B), _ptr(value_loss)))

    def trpo_get_report(self, learner) -> dict:
        """What the last policy step did (ev2g_trpo_report's fields).  Synchronises."""
        rep = _abi.TrpoReportC()
        self._check(self._lib.ev2g_trpo_get_report(self._h, learner, C.byref(rep)))
        return {k: getattr(rep, k) for k, _ in _abi.TrpoReportC._fields_}

    def trpo_get_direction(self, learner, n_actor):
        """(x, g) of the last policy step as host float64 arrays [n_actor], flat in the actor's order.  Synchronises."""
        x, g = np.empty(n_actor, np.float64), np.empty(n_actor, np.float64)
        self._check(self._lib.ev2g_trpo_get_direction(self._h, learner, x.ctypes.data, g.ctypes.data))
        return x, g

    # ---- the TD3 / DDPG learner and the replay ring's sampler (include/ev2g.h: ev2g_td3_*, ev2g_replay_sample) ------------------------------
    def td3_create(self, mlp, actor, critics, seed=0, ddpg=False, **config):
        """A TD3 (or, ddpg=True, DDPG) learner bound to the policy `mlp` (ev2g_td3_create): actor six host arrays, critics a list of six-array
        lists; config overrides fields of the preset (ev2g_td3_config).  Freed by td3_destroy, with its policy or with the engine."""
        cfg = td3_default_config(ddpg)
        for k, v in config.items():
            if k not in dict(_abi.Td3ConfigC._fields_):
                raise TypeError(f"td3_create: unknown config field {k}")
            setattr(cfg, k, int(v) if k in ("n_critics", "policy_delay") else float(v))
        actor = [np.ascontiguousarray(a, np.float32) for a in actor]
        flat = [np.ascontiguousarray(a, np.float32) for c in critics for a in c]
        if len(actor) != 6 or len(flat) != 6 * cfg.n_critics:
            raise ValueError(f"td3_create: six actor arrays and six per critic for {cfg.n_critics} critics are needed")
        (h1, d_in), h2, d_out = actor[0].shape, actor[2].shape[0], actor[4].shape[0]
        for a, shape in zip(actor + flat, _abi.td3_param_shapes(d_in, h1, h2, d_out, cfg.n_critics)):
            if a.shape != shape:
                raise ValueError(f"td3_create: a weight array has shape {a.shape}, expected {shape}")
        pa, pc = (C.c_void_p * 6)(*[a.ctypes.data for a in actor]), (C.c_void_p * len(flat))(*[a.ctypes.data for a in flat])
        out = C.c_void_p()
        self._check(self._lib.ev2g_td3_create(self._h, mlp, C.byref(cfg), d_in, h1, h2, d_out, pa, pc, int(seed) & (2 ** 64 - 1), C.byref(out)))
        return out.value

    def td3_destroy(self, t):
        if t and self._h:
            self._lib.ev2g_td3_destroy(self._h, t)

    def td3_update(self, t, obs, actions, reward, next_obs, done, B, losses=None):
        """One gradient step on contiguous DEVICE batch arrays (ev2g_td3_update); losses: float32 [2] DEVICE or None."""
        self._check(self._lib.ev2g_td3_update(self._h, t, _ptr(obs), _ptr(actions), _ptr(reward), _ptr(next_obs), _ptr(done), int(B), _ptr(losses)))

    def td3_critic_grad(self, t, obs, actions, reward, next_obs, done, B, losses=None):
        self._check(self._lib.ev2g_td3_critic_grad(self._h, t, _ptr(obs), _ptr(actions), _ptr(reward), _ptr(next_obs), _ptr(done), int(B), _ptr(losses)))

    def td3_actor_grad(self, t, obs, B, losses=None):
        self._check(self._lib.ev2g_td3_actor_grad(self._h, t, _ptr(obs), int(B), _ptr(losses)))

    def td3_apply(self, t):
        self._check(self._lib.ev2g_td3_apply(self._h, t))

    def _td3_arrays(self, entry, t, shape, *args):
        out = [np.empty(s, np.float32) for s in _abi.td3_param_shapes(*shape)]
        self._check(getattr(self._lib, entry)(self._h, t, *args, (C.c_void_p * len(out))(*[a.ctypes.data for a in out])))
        return out

    def td3_get_grads(self, t, shape):
        """The last gradient of each half as 6 + 6 n_critics host float32 arrays; shape: (d_in, h1, h2, d_out, n_critics)."""
        return self._td3_arrays("ev2g_td3_get_grads", t, shape)

    def td3_get_weights(self, t, shape, target=False):
        """The masters (or the target networks) as 6 + 6 n_critics host float32 arrays in SB3's parameter order."""
        return self._td3_arrays("ev2g_td3_get_weights", t, shape, int(bool(target)))

    def td3_get_y(self, t, B):
        y = np.empty(int(B), np.float32)
        self._check(self._lib.ev2g_td3_get_y(self._h, t, y.ctypes.data, int(B)))
        return y

    def td3_set_rate(self, t, lr):
        self._check(self._lib.ev2g_td3_set_rate(self._h, t, float(lr)))

    def td3_seed(self, t, seed, first_draw=0):
        self._check(self._lib.ev2g_td3_seed(self._h, t, int(seed) & (2 ** 64 - 1), int(first_draw)))

    def td3_counters(self, t):
        """(updates applied to the critics, actor steps, the next noise draw index)."""
        n, a, d = C.c_int64(0), C.c_int64(0), C.c_uint64(0)
        self._check(self._lib.ev2g_td3_counters(self._h, t, C.byref(n), C.byref(a), C.byref(d)))
        return int(n.value), int(a.value), int(d.value)

    def replay_sample(self, blocks, T, E, D, P, B, seed, counter, obs, actions, reward, next_obs, done, index=None):
        """Draw `counter` of B uniform transitions from the COMPLETE episode blocks `blocks` (a list of (obs, actions, reward, done) device arrays)
        into the contiguous DEVICE batch arrays (ev2g_replay_sample); index: int32 [B, 3] DEVICE or None."""
        cols = [(C.c_void_p * len(blocks))(*[_ptr(b[i]) for b in blocks]) for i in range(4)]
        ring = _abi.ReplayRingC(len(blocks), int(T), int(E), int(D), int(P), *[C.cast(c, C.c_void_p) for c in cols])
        self._check(self._lib.ev2g_replay_sample(self._h, C.byref(ring), int(B), int(seed) & (2 ** 64 - 1), int(counter), _ptr(obs), _ptr(actions),
                                                 _ptr(reward), _ptr(next_obs), _ptr(done), _ptr(index)))

    # ---- the SAC learner and its collection actor (include/ev2g.h: ev2g_sac_*) ----------------------------------------------------------------
    def sac_create(self, actor, critics, lo, seed=0, **config):
        """A SAC learner with its stochastic collection actor (ev2g_sac_create): actor eight host arrays, critics a list of six-array lists;
        config overrides fields of SB3's defaults (ev2g_sac_config).  Freed by sac_destroy or with the engine."""
        cfg = sac_default_config()
        ints = ("n_critics", "target_update_interval", "ent_coef_auto", "target_entropy_auto")
        for k, v in config.items():
            if k not in dict(_abi.SacConfigC._fields_):
                raise TypeError(f"sac_create: unknown config field {k}")
            setattr(cfg, k, int(v) if k in ints else float(v))
        actor = [np.ascontiguousarray(a, np.float32) for a in actor]
        flat = [np.ascontiguousarray(a, np.float32) for c in critics for a in c]
        if len(actor) != 8 or len(flat) != 6 * cfg.n_critics:
            raise ValueError(f"sac_create: eight actor arrays and six per critic for {cfg.n_critics} critics are needed")
        (h1, d_in), h2, d_out = actor[0].shape, actor[2].shape[0], actor[4].shape[0]
        for a, shape in zip(actor + flat, _abi.sac_param_shapes(d_in, h1, h2, d_out, cfg.n_critics)):
            if a.shape != shape:
                raise ValueError(f"sac_create: a weight array has shape {a.shape}, expected {shape}")
        pa, pc = (C.c_void_p * 8)(*[a.ctypes.data for a in actor]), (C.c_void_p * len(flat))(*[a.ctypes.data for a in flat])
        out = C.c_void_p()
        self._check(self._lib.ev2g_sac_create(self._h, C.byref(cfg), d_in, h1, h2, d_out, float(lo), pa, pc, int(seed) & (2 ** 64 - 1), C.byref(out)))
        return out.value

    def sac_destroy(self, s):
        if s and self._h:
            self._lib.ev2g_sac_destroy(self._h, s)

    def sac_update(self, s, obs, actions, reward, next_obs, done, B, losses=None):
        """One gradient step on contiguous DEVICE batch arrays (ev2g_sac_update); losses: float32 [4] DEVICE or None."""
        self._check(self._lib.ev2g_sac_update(self._h, s, _ptr(obs), _ptr(actions), _ptr(reward), _ptr(next_obs), _ptr(done), int(B), _ptr(losses)))

    def sac_critic_grad(self, s, obs, actions, reward, next_obs, done, B, losses=None):
        self._check(self._lib.ev2g_sac_critic_grad(self._h, s, _ptr(obs), _ptr(actions), _ptr(reward), _ptr(next_obs), _ptr(done), int(B), _ptr(losses)))

    def sac_actor_grad(self, s, obs, B, losses=None):
        self._check(self._lib.ev2g_sac_actor_grad(self._h, s, _ptr(obs), int(B), _ptr(losses)))

    def sac_apply(self, s):
        self._check(self._lib.ev2g_sac_apply(self._h, s))

    def sac_act(self, s, obs32, n_rows, actions, deterministic=False, mu=None, log_std=None, log_pi=None):
        """The collection actor on n_rows DEVICE observation rows (ev2g_sac_act): env actions in [lo, 1]; mu, raw log_std, log pi optional."""
        self._check(self._lib.ev2g_sac_act(self._h, s, _ptr(obs32), int(n_rows), int(bool(deterministic)), _ptr(actions), _ptr(mu), _ptr(log_std), _ptr(log_pi)))

    def sac_collect(self, s, k, obs, actions, reward, done, mask, deterministic=False):
        """k x (SAC actor -> env step) into the caller's DEVICE arrays (ev2g_sac_collect; the arrays of collect())."""
        tr = (C.c_void_p * 5)(_ptr(obs), _ptr(actions), _ptr(reward), _ptr(done), _ptr(mask))
        self._check(self._lib.ev2g_sac_collect(self._h, s, int(k), int(bool(deterministic)), C.cast(tr, C.c_void_p)))

    def sac_get_grads(self, s, shape):
        """(the last gradient of each half as 8 + 6 n_critics host float32 arrays, the gradient of log_ent_coef); shape: (d_in, h1, h2, d_out, n_critics)."""
        out = [np.empty(sh, np.float32) for sh in _abi.sac_param_shapes(*shape)]
        g = np.zeros(1, np.float32)
        self._check(self._lib.ev2g_sac_get_grads(self._h, s, (C.c_void_p * len(out))(*[a.ctypes.data for a in out]), g.ctypes.data))
        return out, float(g[0])

    def sac_get_weights(self, s, shape, target=False):
        """The masters as 8 + 6 n_critics host float32 arrays in SB3's parameter order, or (target) the target critics' 6 n_critics."""
        out = [np.empty(sh, np.float32) for sh in _abi.sac_param_shapes(*shape)]
        self._check(self._lib.ev2g_sac_get_weights(self._h, s, int(bool(target)), (C.c_void_p * len(out))(*[a.ctypes.data for a in out])))
        return out[8:] if target else out

    def sac_get_y(self, s, B):
        """(y, log pi') of the last critic gradient."""
        y, lp = np.empty(int(B), np.float32), np.empty(int(B), np.float32)
        self._check(self._lib.ev2g_sac_get_y(self._h, s, y.ctypes.data, lp.ctypes.data, int(B)))
        return y, lp

    def sac_get_log_pi(self, s, B):
        lp = np.empty(int(B), np.float32)
        self._check(self._lib.ev2g_sac_get_log_pi(self._h, s, lp.ctypes.data, int(B)))
        return lp

    def sac_get_ent_coef(self, s):
        """float32 [3]: log_ent_coef and its Adam moments m, v."""
        out = np.empty(3, np.float32)
        self._check(self._lib.ev2g_sac_get_ent_coef(self._h, s, out.ctypes.data))
        return out

    def sac_set_rate(self, s, lr):
        self._check(self._lib.ev2g_sac_set_rate(self._h, s, float(lr)))

    def sac_seed(self, s, seed, first_draw=0):
        self._check(self._lib.ev2g_sac_seed(self._h, s, int(seed) & (2 ** 64 - 1), int(first_draw)))

    def sac_act_seed(self, s, seed, first_launch=0):
        self._check(self._lib.ev2g_sac_act_seed(self._h, s, int(seed) & (2 ** 64 - 1), int(first_launch)))

    def sac_counters(self, s):
        """(updates applied, Polyak steps among them, the learner's next draw base, the collection stream's launch counter)."""
        n, t, d, a = C.c_int64(0), C.c_int64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.ev2g_sac_counters(self._h, s, C.byref(n), C.byref(t), C.byref(d), C.byref(a)))
        return int(n.value), int(t.value), int(d.value), int(a.value)

    # ---- the TQC learner and its collection actor (include/ev2g.h: ev2g_tqc_*) ----------------------------------------------------------------
    def tqc_create(self, actor, critics, lo, seed=0, **config):
        """A TQC learner with its stochastic collection actor (ev2g_tqc_create): actor eight host arrays, critics a list of six-array lists
        (the last layer with n_quantiles rows); config overrides fields of sb3_contrib's defaults (ev2g_tqc_config).  Freed by tqc_destroy or
        with the engine."""
        cfg = tqc_default_config()
        ints = ("n_critics", "target_update_interval", "ent_coef_auto", "target_entropy_auto", "n_quantiles", "top_quantiles_to_drop_per_net")
        for k, v in config.items():
            if k not in dict(_abi.TqcConfigC._fields_):
                raise TypeError(f"tqc_create: unknown config field {k}")
            setattr(cfg, k, int(v) if k in ints else float(v))
        actor = [np.ascontiguousarray(a, np.float32) for a in actor]
        flat = [np.ascontiguousarray(a, np.float32) for c in critics for a in c]
        if len(actor) != 8 or len(flat) != 6 * cfg.n_critics:
            raise ValueError(f"tqc_create: eight actor arrays and six per critic for {cfg.n_critics} critics are needed")
        (h1, d_in), h2, d_out = actor[0].shape, actor[2].shape[0], actor[4].shape[0]
        for a, shape in zip(actor + flat, _abi.tqc_param_shapes(d_in, h1, h2, d_out, cfg.n_critics, cfg.n_quantiles)):
            if a.shape != shape:
                raise ValueError(f"tqc_create: a weight array has shape {a.shape}, expected {shape}")
        pa, pc = (C.c_void_p * 8)(*[a.ctypes.data for a in actor]), (C.c_void_p * max(len(flat), 1))(*[a.ctypes.data for a in flat])
        out = C.c_void_p()
        self._check(self._lib.ev2g_tqc_create(self._h, C.byref(cfg), d_in, h1, h2, d_out, float(lo), pa, pc, int(seed) & (2 ** 64 - 1), C.byref(out)))
        return out.value

    def tqc_destroy(self, t):
        if t and self._h:
            self._lib.ev2g_tqc_destroy(self._h, t)

    def tqc_update(self, t, obs, actions, reward, next_obs, done, B, losses=None):
        """One gradient step on contiguous DEVICE batch arrays (ev2g_tqc_update); losses: float32 [4] DEVICE or None."""
        self._check(self._lib.ev2g_tqc_update(self._h, t, _ptr(obs), _ptr(actions), _ptr(reward), _ptr(next_obs), _ptr(done), int(B), _ptr(losses)))

    def tqc_critic_grad(self, t, obs, actions, reward, next_obs, done, B, losses=None):
        self._check(self._lib.ev2g_tqc_critic_grad(self._h, t, _ptr(obs), _ptr(actions), _ptr(reward), _ptr(next_obs), _ptr(done), int(B), _ptr(losses)))

    def tqc_actor_grad(self, t, obs, B, losses=None):
        self._check(self._lib.ev2g_tqc_actor_grad(self._h, t, _ptr(obs), int(B), _ptr(losses)))

    def tqc_apply(self, t):
        self._check(self._lib.ev2g_tqc_apply(self._h, t))

    def tqc_act(self, t, obs32, n_rows, actions, deterministic=False, mu=None, log_std=None, log_pi=None):
        """The collection actor on n_rows DEVICE observation rows (ev2g_tqc_act): env actions in [lo, 1]; mu, raw log_std, log pi optional."""
        self._check(self._lib.ev2g_tqc_act(self._h, t, _ptr(obs32), int(n_rows), int(bool(deterministic)), _ptr(actions), _ptr(mu), _ptr(log_std), _ptr(log_pi)))

    def tqc_collect(self, t, k, obs, actions, reward, done, mask, deterministic=False):
        """k x (TQC actor -> env step) into the caller's DEVICE arrays (ev2g_tqc_collect; the arrays of collect())."""
        tr = (C.c_void_p * 5)(_ptr(obs), _ptr(actions), _ptr(reward), _ptr(done), _ptr(mask))
        self._check(self._lib.ev2g_tqc_collect(self._h, t, int(k), int(bool(deterministic)), C.cast(tr, C.c_void_p)))

    def tqc_get_grads(self, t, shape):
        """(the last gradient of each half as 8 + 6 n_critics host float32 arrays, the gradient of log_ent_coef); shape: (d_in, h1, h2, d_out,
        n_critics, n_quantiles)."""
        out = [np.empty(sh, np.float32) for sh in _abi.tqc_param_shapes(*shape)]
        g = np.zeros(1, np.float32)
        self._check(self._lib.ev2g_tqc_get_grads(self._h, t, (C.c_void_p * len(out))(*[a.ctypes.data for a in out]), g.ctypes.data))
        return out, float(g[0])

    def tqc_get_weights(self, t, shape, target=False):
        """The masters as 8 + 6 n_critics host float32 arrays in sb3_contrib's parameter order, or (target) the target critics' 6 n_critics."""
        out = [np.empty(sh, np.float32) for sh in _abi.tqc_param_shapes(*shape)]
        self._check(self._lib.ev2g_tqc_get_weights(self._h, t, int(bool(target)), (C.c_void_p * len(out))(*[a.ctypes.data for a in out])))
        return out[8:] if target else out

    def tqc_get_z(self, t, B, K):
        """(z [B, K], log pi' [B]) of the last critic gradient."""
        z, lp = np.empty((int(B), int(K)), np.float32), np.empty(int(B), np.float32)
        self._check(self._lib.ev2g_tqc_get_z(self._h, t, z.ctypes.data, lp.ctypes.data, int(B)))
        return z, lp

    def tqc_get_log_pi(self, t, B):
        lp = np.empty(int(B), np.float32)
        self._check(self._lib.ev2g_tqc_get_log_pi(self._h, t, lp.ctypes.data, int(B)))
        return lp

    def tqc_get_ent_coef(self, t):
        """float32 [3]: log_ent_coef and its Adam moments m, v."""
        out = np.empty(3, np.float32)
        self._check(self._lib.ev2g_tqc_get_ent_coef(self._h, t, out.ctypes.data))
        return out

    def tqc_set_rate(self, t, lr):
        self._check(self._lib.ev2g_tqc_set_rate(self._h, t, float(lr)))

    def tqc_seed(self, t, seed, first_draw=0):
        self._check(self._lib.ev2g_tqc_seed(self._h, t, int(seed) & (2 ** 64 - 1), int(first_draw)))

    def tqc_act_seed(self, t, seed, first_launch=0):
        self._check(self._lib.ev2g_tqc_act_seed(self._h, t, int(seed) & (2 ** 64 - 1), int(first_launch)))

    def tqc_counters(self, t):
        """(updates applied, Polyak steps among them, the learner's next draw base, the collection stream's launch counter)."""
        n, tu, d, a = C.c_int64(0), C.c_int64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.ev2g_tqc_counters(self._h, t, C.byref(n), C.byref(tu), C.byref(d), C.byref(a)))
        return int(n.value), int(tu.value), int(d.value), int(a.value)

    def tqc_truncate(self, tq, log_pi_next, reward, done, B, n_critics, n_quantiles, drop, gamma, log_ent_coef, z_out):
        """The sort-and-truncate kernel alone on DEVICE arrays (ev2g_tqc_truncate): tq [n_critics][B, n_quantiles] -> z_out [B, K]."""
        self._check(self._lib.ev2g_tqc_truncate(self._h, _ptr(tq), _ptr(log_pi_next), _ptr(reward), _ptr(done), int(B), int(n_critics), int(n_quantiles), int(drop),
                                                float(gamma), _ptr(log_ent_coef), _ptr(z_out)))

    # ---- the ARS learner and its population actor (include/ev2g.h: ev2g_ars_*) ------------------------------------------------------------------
    def ars_create(self, kind, d_in, h1, h2, d_out, lo, theta=None, seed=0, **config):
        """An ARS learner (ev2g_ars_create): kind "MlpPolicy" or "LinearPolicy"; theta float32 [n_params] or None for zeros; config overrides
        fields of sb3_contrib's defaults (ev2g_ars_config).  Freed by ars_destroy or with the engine."""
        cfg = ars_config(**config)
        th = None if theta is None else np.ascontiguousarray(theta, np.float32)
        n = ars_query(kind, d_in, h1, h2, d_out, cfg)["n_params"]
        if th is not None and th.shape != (n,):
            raise ValueError(f"ars_create: theta has shape {th.shape}, expected {(n,)}")
        out = C.c_void_p()
        self._check(self._lib.ev2g_ars_create(self._h, C.byref(cfg), _abi.ARS_KINDS[kind], int(d_in), int(h1), int(h2), int(d_out), float(lo),
                                              None if th is None else th.ctypes.data, int(seed) & (2 ** 64 - 1), C.byref(out)))
        return out

    def ars_destroy(self, a):
        if a and self._h:
            self._lib.ev2g_ars_destroy(self._h, a)

    def ars_perturb(self, a):
        self._check(self._lib.ev2g_ars_perturb(self._h, a))

    def ars_act(self, a, obs32, n_rows, actions, population=False):
        """DEVICE obs32 [n_rows, D] -> actions [n_rows, P] (ev2g_ars_act): under theta, or rows [c R, (c + 1) R) under candidate c."""
        self._check(self._lib.ev2g_ars_act(self._h, a, _ptr(obs32), int(n_rows), int(bool(population)), _ptr(actions)))

    def ars_obs_f32(self, a) -> int:
        p = self._lib.ev2g_ars_obs_f32(self._h, a)
        if not p:
            self._check(_abi.ERR_STATE)
        return p

    def ars_actions_f32(self, a) -> int:
        p = self._lib.ev2g_ars_actions_f32(self._h, a)
        if not p:
            self._check(_abi.ERR_STATE)
        return p

    def ars_rollout(self, a, k, population=True, reward=None, r_stride=0):
        """k x (population or centre actor -> env step) from the object's observation row (ev2g_ars_rollout)."""
        self._check(self._lib.ev2g_ars_rollout(self._h, a, int(k), int(bool(population)), _ptr(reward), int(r_stride)))

    def ars_update(self, a):
        self._check(self._lib.ev2g_ars_update(self._h, a))

    def ars_get_report(self, a, n_delta) -> dict:
        rep, ret, ranks = _abi.ArsReportC(), np.empty(2 * int(n_delta), np.float64), np.empty(int(n_delta), np.int32)
        self._check(self._lib.ev2g_ars_get_report(self._h, a, C.byref(rep), ret.ctypes.data, ranks.ctypes.data))
        return dict(returns=ret, ranks=ranks, sigma_r=rep.sigma_r, step=rep.step, refused=bool(rep.refused), first_bad=rep.first_bad, n_top=rep.n_top,
                    iteration=rep.iteration)

    def ars_get_weights(self, a, n_params):
        th = np.empty(int(n_params), np.float32)
        self._check(self._lib.ev2g_ars_get_weights(self._h, a, th.ctypes.data))
        return th

    def ars_set_weights(self, a, theta):
        th = np.ascontiguousarray(theta, np.float32)
        self._check(self._lib.ev2g_ars_set_weights(self._h, a, th.ctypes.data))

    def ars_get_candidate(self, a, c, n_params):
        th = np.empty(int(n_params), np.float32)
        self._check(self._lib.ev2g_ars_get_candidate(self._h, a, int(c), th.ctypes.data))
        return th

    def ars_get_deltas(self, a, n_delta, n_params):
        d = np.empty((int(n_delta), int(n_params)), np.float32)
        self._check(self._lib.ev2g_ars_get_deltas(self._h, a, d.ctypes.data))
        return d

    def ars_get_env_returns(self, a):
        r = np.empty(self.E, np.float64)
        self._check(self._lib.ev2g_ars_get_env_returns(self._h, a, r.ctypes.data, self.E))
        return r

    def ars_set_returns(self, a, returns):
        r = np.ascontiguousarray(returns, np.float64)
        self._check(self._lib.ev2g_ars_set_returns(self._h, a, r.ctypes.data))

    def ars_set_rates(self, a, learning_rate, delta_std):
        self._check(self._lib.ev2g_ars_set_rates(self._h, a, float(learning_rate), float(delta_std)))

    def ars_seed(self, a, seed, first_iteration=0):
        self._check(self._lib.ev2g_ars_seed(self._h, a, int(seed) & (2 ** 64 - 1), int(first_iteration)))

    def ars_counters(self, a):
        """(the next perturb's iteration, updates queued, env steps since the last perturb)"""
        n, u, st = C.c_uint64(), C.c_int64(), C.c_int64()
        self._check(self._lib.ev2g_ars_counters(self._h, a, C.byref(n), C.byref(u), C.byref(st)))
        return n.value, u.value, st.value

    def stats(self, out=None) -> np.ndarray:
        """[E,17] get_statistics() scalars (utils.py:84-101) as a host array (or into a device `out`)."""
        if out is not None:
            self._check(self._lib.ev2g_get_stats(self._h, _ptr(out)))
            return out
        buf = self.empty((self.E, _abi.N_STATS))
        try:
            self._check(self._lib.ev2g_get_stats(self._h, buf.ptr))
            return buf.to_host()
        finally:
            buf.free()

    def collect(self, m, k, obs, actions, reward, done, mask):
        """k x (actor forward -> env step) with the transitions written straight into the caller's DEVICE arrays (ev2g_collect):
        obs float32 [k + 1, E, D] (row 0 is the input observation), actions float32 [k, E, P], reward float64 [k, E], done / mask uint8."""
        class _Tr(C.Structure):
            _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("mask", C.c_void_p)]
        tr = _Tr(_ptr(obs), _ptr(actions), _ptr(reward), _ptr(done), _ptr(mask))
        self._check(self._lib.ev2g_collect(self._h, m, int(k), C.byref(tr)))

    def reset_f32(self, obs32=None, offset: int = 0):
        self._check(self._lib.ev2g_reset_f32(self._h, _ptr(obs32), int(offset)))

    def stats_reset_f32(self, out, obs32=None, offset: int = 0):
        self._check(self._lib.ev2g_get_stats_reset_f32(self._h, _ptr(out), _ptr(obs32), int(offset)))
        return out

    def stats_reset(self, out, obs=None, offset: int = 0):
        """Episode end in one launch: get_statistics() of the finished episode into the device buffer `out`, then reset() onto the pool
        window `offset` (reset observation into `obs`) -- ev2g_get_stats_reset."""
        self._check(self._lib.ev2g_get_stats_reset(self._h, _ptr(out), _ptr(obs), int(offset)))
        return out

    # ---- multi-GPU statistics exchange over RCCL (include/ev2g.h: ev2g_comm_*, ev2g_gather_stats) ----
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: the communicator id to hand to every rank's comm_init (128 bytes; ship them by any host-side channel)."""
        buf = C.create_string_buffer(_abi.COMM_ID_BYTES)
        rc = load_library().ev2g_comm_get_unique_id(C.cast(buf, C.c_void_p))
        if rc:
            raise EngineError(rc, (load_library().ev2g_last_error(None) or b"").decode())
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world_size: int):
        assert len(unique_id) == _abi.COMM_ID_BYTES
        buf = C.create_string_buffer(unique_id, _abi.COMM_ID_BYTES)
        self._check(self._lib.ev2g_comm_init(self._h, C.cast(buf, C.c_void_p), int(rank), int(world_size)))

    @property
    def comm_world_size(self) -> int:
        return int(self._lib.ev2g_comm_world_size(self._h))

    @property
    def comm_gathers(self) -> int:
        return int(self._lib.ev2g_comm_gathers(self._h))

    def gather_stats(self, out=None) -> np.ndarray:
        """Episode statistics of every rank, [world*E,17] rank-major: this rank's statistics kernel followed by ncclAllGather on the
        engine's stream.  Into the device array `out` (asynchronous), or returned as a host array."""
        if out is not None:
            self._check(self._lib.ev2g_gather_stats(self._h, _ptr(out)))
            return out
        buf = self.empty((self.comm_world_size * self.E, _abi.N_STATS))
        try:
            self._check(self._lib.ev2g_gather_stats(self._h, buf.ptr))
            return buf.to_host()
        finally:
            buf.free()

    # ---- scenario generation on the device ---------------------------------------------------------
    def pool_refill(self, gen_cfg, seed: int, first_index: int, first_slot: int, n: int):
        """Re-draw pool slots [first_slot, first_slot + n) ON THE DEVICE as scenarios first_index.. of the stream (gen_cfg, seed): bit for
        bit what `generate_native(gen_cfg with that seed)` yields at those indices (include/ev2g.h: ev2g_pool_refill).  The engine must have
        been created with FLAG_REFILLABLE from a batch drawn with the same config.  Asynchronous; refill slots no env is stepping."""
        from .scenario_gen import gen_config_c
        c, keep = gen_config_c(gen_cfg)
        self._check(self._lib.ev2g_pool_refill(self._h, C.byref(c), int(seed) & (2 ** 64 - 1), int(first_index), int(first_slot), int(n)))
        self.batch_is_stale = True
        del keep

    @property
    def pool_refill_overflows(self) -> int:
        return int(self._lib.ev2g_pool_refill_overflows(self._h))

    @property
    def pool_session_capacity(self) -> int:
        return int(self._lib.ev2g_pool_session_capacity(self._h))

    def peek(self, env: int = 0) -> dict:
        """Host copy of one env's state in the reference's port order (feeds the EV2Gym facade)."""
        P, Cn, R, T = self.P, self.C, self.R, self.T
        st = self.batch.arrays["env_session_start"]
        scn = (env + self.scenario_offset) % self.M   # the scenario this env is running
        S = int(st[scn + 1] - st[scn])
        f8 = lambda *s: np.empty(s, np.float64)  # noqa: E731
        i4 = lambda *s: np.empty(s, np.int32)  # noqa: E731
        d = dict(port_capacity=f8(P), port_energy=f8(P), port_current=f8(P), port_total_energy=f8(P),
                 port_required_energy=f8(P), port_prev_power=f8(P), port_cycles=i4(P), port_session=i4(P),
                 cs_power=f8(Cn), cs_amps=f8(Cn), cs_profits=f8(Cn), cs_energy_charged=f8(Cn),
                 cs_energy_discharged=f8(Cn), tr_power=f8(R), tr_overload=f8(R, T), power_usage=f8(T),
                 power_potential=f8(T), session_port=i4(max(S, 1)), session_afap=f8(max(S, 1)),
                 session_final_cap=f8(max(S, 1)))
        v = _abi.EnvViewC()
        for k, a in d.items():
            ct = C.c_double if a.dtype == np.float64 else C.c_int32
            setattr(v, k, a.ctypes.data_as(C.POINTER(ct)))
        self._check(self._lib.ev2g_peek(self._h, int(env), C.byref(v)))
        d["session_port"] = d["session_port"][:S]
        d["session_afap"] = d["session_afap"][:S]
        d["session_final_cap"] = d["session_final_cap"][:S]
        d["current_step"] = int(v.current_step)
        return d

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ev2g_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_uniform(n, seed, lo, hi) -> np.ndarray:
    """Host twin of Engine.fill_uniform (same counter-based generator)."""
    out = np.empty(int(n))
    load_library().ev2g_host_uniform(out.ctypes.data, int(n), int(seed), float(lo), float(hi))
    return out


def host_normal(n, seed, first_index=0) -> np.ndarray:
    """Host twin of the actor-critic's noise (ev2g_ac_host_normal): the float32 standard normals of draw indices first_index .. + n - 1."""
    out = np.empty(int(n), np.float32)
    load_library().ev2g_ac_host_normal(out.ctypes.data, int(n), int(seed) & (2 ** 64 - 1), int(first_index))
    return out


def host_gae(reward, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
    """Host twin of Engine.gae (ev2g_host_gae, the same source): [k, n_envs] host arrays -> (advantages, returns) float32."""
    reward = np.ascontiguousarray(reward, np.float64)
    values = np.ascontiguousarray(values, np.float32)
    starts = np.ascontiguousarray(episode_starts, np.uint8)
    lv, ld = np.ascontiguousarray(last_values, np.float32), np.ascontiguousarray(last_dones, np.uint8)
    k, n = reward.shape
    assert values.shape == (k, n) and starts.shape == (k, n) and lv.shape == (n,) and ld.shape == (n,)
    adv, ret = np.empty((k, n), np.float32), np.empty((k, n), np.float32)
    rc = load_library().ev2g_host_gae(reward.ctypes.data, values.ctypes.data, starts.ctypes.data, lv.ctypes.data, ld.ctypes.data, k, n,
                                      float(gamma), float(gae_lambda), adv.ctypes.data, ret.ctypes.data)
    if rc != 0:
        raise EngineError(rc, (load_library().ev2g_last_error(None) or b"").decode())
    return adv, ret


def ppo_query(d_in, h1, h2, v1, v2, d_out) -> dict:
    """The learner's plan of a network (ev2g_ppo_query; host-only): lds_bytes, workspace_bytes, grid_cap, n_params.  EngineError if refused."""
    L = load_library()
    info = _abi.PpoInfoC()
    rc = L.ev2g_ppo_query(int(d_in), int(h1), int(h2), int(v1), int(v2), int(d_out), C.byref(info))
    if rc != 0:
        raise EngineError(rc, L.ev2g_last_error(None).decode())
    return {k: int(getattr(info, k)) for k, _ in _abi.PpoInfoC._fields_}


def trpo_query(d_in, h1, h2, v1, v2, d_out) -> dict:
    """The TRPO learner's plan of a network (ev2g_trpo_query; host-only): lds_bytes, workspace_bytes, grid_cap, n_params, n_actor."""
    L = load_library()
    info = _abi.TrpoInfoC()
    rc = L.ev2g_trpo_query(int(d_in), int(h1), int(h2), int(v1), int(v2), int(d_out), C.byref(info))
    if rc != 0:
        raise EngineError(rc, L.ev2g_last_error(None).decode())
    return {k: int(getattr(info, k)) for k, _ in _abi.TrpoInfoC._fields_}


def host_trpo_cg_step(x, r, p, Hp, rho, last=False):
    """Host twin of one conjugate-gradient iteration (ev2g_host_trpo_cg_step): float64 arrays x / r / p are updated IN PLACE from the given Hp.
    Returns (the new rho, whether the solve has ended)."""
    for a in (x, r, p):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    Hp = np.ascontiguousarray(Hp, np.float64)
    L = load_library()
    rho_c, done = C.c_double(float(rho)), C.c_int32(0)
    rc = L.ev2g_host_trpo_cg_step(x.ctypes.data, r.ctypes.data, p.ctypes.data, Hp.ctypes.data, x.size, C.addressof(rho_c), int(bool(last)),
                                  C.addressof(done))
    if rc != 0:
        raise EngineError(rc, L.ev2g_last_error(None).decode())
    return rho_c.value, bool(done.value)


def host_trpo_rows(mean, mean0, actions, log_std, log_std0, old_log_prob, advantages, normalize_advantage=True):
    """Host twin of the line search's row terms (ev2g_host_trpo_rows): (j [B], kl [B]) float64."""
    mean, mean0, actions, log_std, log_std0, old, adv = (np.ascontiguousarray(a, np.float32) for a in
                                                         (mean, mean0, actions, log_std, log_std0, old_log_prob, advantages))
    B, P = mean.shape
    j, kl = np.empty(B, np.float64), np.empty(B, np.float64)
    L = load_library()
    rc = L.ev2g_host_trpo_rows(mean.ctypes.data, mean0.ctypes.data, actions.ctypes.data, log_std.ctypes.data, log_std0.ctypes.data, old.ctypes.data,
                               adv.ctypes.data, B, P, int(bool(normalize_advantage)), j.ctypes.data, kl.ctypes.data)
    if rc != 0:
        raise EngineError(rc, L.ev2g_last_error(None).decode())
    return j, kl


def host_adam(theta, m, v, g, t, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5):
    """Host twin of the learner's Adam (ev2g_host_adam, the device's element function): float32 arrays theta / m / v are updated IN PLACE."""
    for a in (theta, m, v):
        assert a.dtype == np.float32 and a.flags.c_contiguous
    g = np.ascontiguousarray(g, np.float32)
    L = load_library()
    rc = L.ev2g_host_adam(theta.ctypes.data, m.ctypes.data, v.ctypes.data, g.ctypes.data, theta.size, int(t), float(lr), float(beta1), float(beta2),
                          float(eps))
    if rc != 0:
        raise EngineError(rc, L.ev2g_last_error(None).decode())


def _host_head(entry, cfg, mean, *rows):
    """A host twin of the gradient kernel's head: stages mean [B, P] and `rows` (the entry's arrays after mean, in its order) as float32,
    allocates (d_mean [B, P], d_value [B], d_log_std [P], stats [6]) and calls `entry` with the config `cfg`."""
    mean, *rows = (np.ascontiguousarray(a, np.float32) for a in (mean, *rows))
    B, P = mean.shape
    out = np.empty((B, P), np.float32), np.empty(B, np.float32), np.empty(P, np.float32), np.empty(6, np.float32)
    L = load_library()
    rc = getattr(L, entry)(mean.ctypes.data, *[a.ctypes.data for a in rows], B, P, C.byref(cfg), *[a.ctypes.data for a in out])
    if rc != 0:
        raise EngineError(rc, L.ev2g_last_error(None).decode())
    return out


def host_ppo_head(mean, value, actions, log_std, old_log_prob, advantages, returns, clip_range=0.2, vf_coef=0.5, ent_coef=0.0,
                  normalize_advantage=True):
    """Host twin of the gradient kernel's head (ev2g_host_ppo_head): (d_mean [B, P], d_value [B], d_log_std [P], stats [6]) float32."""
    cfg = _abi.PpoConfigC(0.0, 0.9, 0.999, 1e-5, float(clip_range), float(vf_coef), float(ent_coef), 0.5, int(bool(normalize_advantage)))
    return _host_head("ev2g_host_ppo_head", cfg, mean, value, actions, log_std, old_log_prob, advantages, returns)


def host_rmsprop(theta, sq, g, lr=7e-4, alpha=0.99, eps=1e-5):
    """Host twin of the A2C learner's RMSprop (ev2g_host_rmsprop, the device's element function): float32 arrays theta / sq are updated IN PLACE."""
    for a in (theta, sq):
        assert a.dtype == np.float32 and a.flags.c_contiguous
    g = np.ascontiguousarray(g, np.float32)
    L = load_library()
    rc = L.ev2g_host_rmsprop(theta.ctypes.data, sq.ctypes.data, g.ctypes.data, theta.size, float(lr), float(alpha), float(eps))
    if rc != 0:
        raise EngineError(rc, L.ev2g_last_error(None).decode())


def host_a2c_head(mean, value, actions, log_std, advantages, returns, vf_coef=0.5, ent_coef=0.0, normalize_advantage=False):
    """Host twin of the gradient kernel's A2C head (ev2g_host_a2c_head): (d_mean [B, P], d_value [B], d_log_std [P], stats [6]) float32."""
    cfg = _abi.A2cConfigC(0.0, 0.99, 1e-5, float(vf_coef), float(ent_coef), 0.5, int(bool(normalize_advantage)), 1)
    return _host_head("ev2g_host_a2c_head", cfg, mean, value, actions, log_std, advantages, returns)


def _host_call(rc):
    if rc != 0:
        raise EngineError(rc, (load_library().ev2g_last_error(None) or b"").decode())


def td3_default_config(ddpg=False):
    """SB3's defaults of TD3, or of DDPG, as an _abi.Td3ConfigC (ev2g_td3_default_config)."""
    cfg = _abi.Td3ConfigC()
    _host_call(load_library().ev2g_td3_default_config(int(bool(ddpg)), C.byref(cfg)))
    return cfg


def host_replay_indices(B, n_blocks, T, E, seed, counter):
    """Host twin of the sampler's draw (ev2g_host_replay_indices): int32 [B, 3] of (entry of the complete list, t, e)."""
    out = np.empty((int(B), 3), np.int32)
    _host_call(load_library().ev2g_host_replay_indices(out.ctypes.data, int(B), int(n_blocks), int(T), int(E), int(seed) & (2 ** 64 - 1), int(counter)))
    return out


def host_td3_target(a_target, tq, reward, done, sigma, clip, gamma, seed, first_draw):
    """Host twin of the target path (ev2g_host_td3_target): (a_next [B, P], y [B] or None when tq is None) float32."""
    a_target = np.ascontiguousarray(a_target, np.float32)
    B, P = a_target.shape
    a_next = np.empty((B, P), np.float32)
    if tq is None:
        _host_call(load_library().ev2g_host_td3_target(a_target.ctypes.data, None, None, None, B, P, 1, float(sigma), float(clip), float(gamma),
                                                       int(seed) & (2 ** 64 - 1), int(first_draw), a_next.ctypes.data, None))
        return a_next, None
    tq, reward, done = np.ascontiguousarray(tq, np.float32), np.ascontiguousarray(reward, np.float32), np.ascontiguousarray(done, np.uint8)
    y = np.empty(B, np.float32)
    _host_call(load_library().ev2g_host_td3_target(a_target.ctypes.data, tq.ctypes.data, reward.ctypes.data, done.ctypes.data, B, P, tq.shape[0], float(sigma),
                                                   float(clip), float(gamma), int(seed) & (2 ** 64 - 1), int(first_draw), a_next.ctypes.data, y.ctypes.data))
    return a_next, y


def host_polyak(target, param, tau):
    """Host twin of the Polyak step (ev2g_host_polyak, the device's element function): float32 `target` is updated IN PLACE."""
    assert target.dtype == np.float32 and target.flags.c_contiguous
    param = np.ascontiguousarray(param, np.float32)
    _host_call(load_library().ev2g_host_polyak(target.ctypes.data, param.ctypes.data, target.size, float(tau)))


def sac_default_config():
    """SB3's defaults of SAC as an _abi.SacConfigC (ev2g_sac_default_config)."""
    cfg = _abi.SacConfigC()
    _host_call(load_library().ev2g_sac_default_config(C.byref(cfg)))
    return cfg


def host_sac_head(mu, log_std, eps, lo=-1.0):
    """Host twin of the squashed-Gaussian head (ev2g_host_sac_head): (a [B, P] tanh, a_env [B, P] in [lo, 1], log pi [B]) float32."""
    mu, log_std, eps = (np.ascontiguousarray(a, np.float32) for a in (mu, log_std, eps))
    B, P = mu.shape
    a, a_env, lp = np.empty((B, P), np.float32), np.empty((B, P), np.float32), np.empty(B, np.float32)
    _host_call(load_library().ev2g_host_sac_head(mu.ctypes.data, log_std.ctypes.data, eps.ctypes.data, B, P, float(lo), a.ctypes.data, a_env.ctypes.data,
                                                 lp.ctypes.data))
    return a, a_env, lp


def host_sac_head_back(mu, log_std, eps, g, log_ent_coef):
    """Host twin of the head's backward (ev2g_host_sac_head_back): (d_mu, d_log_std) [B, P] float32 from g = dQ_min / da."""
    mu, log_std, eps, g = (np.ascontiguousarray(a, np.float32) for a in (mu, log_std, eps, g))
    B, P = mu.shape
    dm, dl = np.empty((B, P), np.float32), np.empty((B, P), np.float32)
    _host_call(load_library().ev2g_host_sac_head_back(mu.ctypes.data, log_std.ctypes.data, eps.ctypes.data, g.ctypes.data, B, P, float(log_ent_coef),
                                                      dm.ctypes.data, dl.ctypes.data))
    return dm, dl


def host_sac_y(tq, log_pi_next, reward, done, gamma, log_ent_coef):
    """Host twin of the target (ev2g_host_sac_y): y [B] float32 from the target critics' values tq [n_critics, B] and log pi' [B]."""
    tq, lp, reward = (np.ascontiguousarray(a, np.float32) for a in (tq, log_pi_next, reward))
    done = np.ascontiguousarray(done, np.uint8)
    y = np.empty(tq.shape[1], np.float32)
    _host_call(load_library().ev2g_host_sac_y(tq.ctypes.data, lp.ctypes.data, reward.ctypes.data, done.ctypes.data, tq.shape[1], tq.shape[0], float(gamma),
                                              float(log_ent_coef), y.ctypes.data))
    return y


def tqc_default_config():
    """sb3_contrib's defaults of TQC as an _abi.TqcConfigC (ev2g_tqc_default_config)."""
    cfg = _abi.TqcConfigC()
    _host_call(load_library().ev2g_tqc_default_config(C.byref(cfg)))
    return cfg


def host_tqc_target(tq, log_pi_next, reward, done, drop, gamma, log_ent_coef):
    """Host twin of the sort-and-truncate kernel (ev2g_host_tqc_target): z [B, K] float32 from the target critics' atoms tq [n_critics, B,
    n_quantiles] and log pi' [B]."""
    tq, lp, reward = (np.ascontiguousarray(a, np.float32) for a in (tq, log_pi_next, reward))
    done = np.ascontiguousarray(done, np.uint8)
    nc, B, nq = tq.shape
    z = np.empty((B, max(nc * (nq - int(drop)), 0)), np.float32)
    _host_call(load_library().ev2g_host_tqc_target(tq.ctypes.data, lp.ctypes.data, reward.ctypes.data, done.ctypes.data, B, nc, nq, int(drop), float(gamma),
                                                   float(log_ent_coef), z.ctypes.data))
    return z


def host_tqc_critic_head(z, q, drop):
    """Host twin of the quantile Huber head (ev2g_host_tqc_critic_head): (dq [n_critics, B, n_quantiles], critic_loss) float32 from z [B, K] and
    the critics' outputs q [n_critics, B, n_quantiles]."""
    z, q = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(q, np.float32)
    nc, B, nq = q.shape
    dq, loss = np.empty_like(q), np.zeros(1, np.float32)
    _host_call(load_library().ev2g_host_tqc_critic_head(z.ctypes.data, q.ctypes.data, B, nc, nq, int(drop), dq.ctypes.data, loss.ctypes.data))
    return dq, float(loss[0])


def ars_config(**config):
    """sb3_contrib's defaults of ARS as an _abi.ArsConfigC (ev2g_ars_default_config), with `config`'s fields over them."""
    cfg = _abi.ArsConfigC()
    _host_call(load_library().ev2g_ars_default_config(C.byref(cfg)))
    for k, v in config.items():
        if not hasattr(cfg, k):
            raise TypeError(f"ars_config: unknown config field {k}")
        setattr(cfg, k, v)
    return cfg


def ars_query(kind, d_in, h1, h2, d_out, cfg=None) -> dict:
    """Limits, n_params, bytes and LDS of an ARS learner of this shape (ev2g_ars_query); a refused shape or config raises EngineError."""
    info = _abi.ArsInfoC()
    _host_call(load_library().ev2g_ars_query(C.byref(cfg if cfg is not None else ars_config()), _abi.ARS_KINDS[kind], int(d_in), int(h1), int(h2), int(d_out),
                                             C.byref(info)))
    return {f[0]: getattr(info, f[0]) for f in _abi.ArsInfoC._fields_}


def host_ars_perturb(theta, n_delta, delta_std, seed, iteration):
    """Host twin of ev2g_ars_perturb (ev2g_host_ars_perturb): (delta [n_delta, n_params], cand [2 n_delta, n_params]) float32."""
    theta = np.ascontiguousarray(theta, np.float32)
    delta, cand = np.empty((int(n_delta), theta.size), np.float32), np.empty((2 * int(n_delta), theta.size), np.float32)
    _host_call(load_library().ev2g_host_ars_perturb(theta.ctypes.data, int(n_delta), theta.size, float(delta_std), int(seed) & (2 ** 64 - 1), int(iteration),
                                                    delta.ctypes.data, cand.ctypes.data))
    return delta, cand


def host_ars_returns(env_return, reward, n_candidates=0, alive_bonus_offset=0.0, steps=0):
    """Host twin of the returns launches (ev2g_host_ars_returns): float64 `env_return` [E] += the rows reward [k, E] (None: nothing) IN PLACE;
    returns the candidates' returns [n_candidates] (None for 0)."""
    assert env_return.dtype == np.float64 and env_return.flags.c_contiguous
    rw = None if reward is None else np.ascontiguousarray(reward, np.float64)
    out = np.empty(int(n_candidates), np.float64) if n_candidates else None
    _host_call(load_library().ev2g_host_ars_returns(env_return.ctypes.data, None if rw is None else rw.ctypes.data, 0 if rw is None else rw.shape[0],
                                                    env_return.size if rw is None else rw.shape[1], env_return.size, int(n_candidates), float(alive_bonus_offset),
                                                    int(steps), None if out is None else out.ctypes.data))
    return out


def host_ars_update(theta, delta, returns, n_top, learning_rate):
    """Host twin of ev2g_ars_update (ev2g_host_ars_update): (new theta float32, report dict as Engine.ars_get_report's)."""
    theta = np.array(theta, np.float32)
    delta, returns = np.ascontiguousarray(delta, np.float32), np.ascontiguousarray(returns, np.float64)
    n_delta = delta.shape[0]
    ranks, rep = np.empty(n_delta, np.int32), _abi.ArsReportC()
    _host_call(load_library().ev2g_host_ars_update(theta.ctypes.data, delta.ctypes.data, returns.ctypes.data, n_delta, int(n_top), theta.size, float(learning_rate),
                                                   ranks.ctypes.data, C.byref(rep)))
    return theta, dict(returns=returns.copy(), ranks=ranks, sigma_r=rep.sigma_r, step=rep.step, refused=bool(rep.refused), first_bad=rep.first_bad, n_top=rep.n_top)
