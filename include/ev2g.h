/*
 * ev2g.h -- C-ABI of the MI355X-native vectorised EV2Gym step engine (libev2g_hip.so).
 *
 * The reference (StavrosOrf/EV2Gym) has no FFI/operator layer for this path; its boundary is the
 * Python class ev2gym.models.ev2gym_env.EV2Gym (constructor :38-56, reset :243-331, step :333-447)
 * plus the rl_agent.state / rl_agent.reward hooks.  Each entry point below names the reference
 * interface it replaces.  Everything is `extern "C"`, plain pointers and sizes, no torch types.
 *
 * Conventions
 *   E envs stepped out of M >= E resident scenarios, C chargers/env, P = sum of the chargers' n_ports
 *   (C * ports_per_charger when they are equal), R transformers/env, T steps/episode, H = 20 observation
 *   horizon (state.py:119,129-132).  All floating point is IEEE float64 (float32 hand-over optional).
 *   Port index p = first port of the charger + port: cumulative in charger order, the reference's action
 *   order (ev2gym_env.py:363-385); the action mask follows the reference's own index i*n_ports+j (:452-457).
 *   Return value: 0 = ok, negative = EV2G_ERR_*; ev2g_last_error() returns a message.
 *   A handle is bound to one GPU and one HIP stream and is not thread-safe; distinct handles may be
 *   driven from distinct threads / processes (one process per GPU).
 *   Unless stated otherwise every `double*` / `uint8_t*` argument of reset/step/get_* is a DEVICE
 *   pointer (hipMalloc'd, or a torch-ROCm tensor's data_ptr()); the scenario batch is HOST memory,
 *   borrowed only for the duration of ev2g_load_scenarios().
 */
#ifndef EV2G_H
#define EV2G_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EV2G_ABI_VERSION 4

/* reward_function built-ins (rl_agent/reward.py) */
#define EV2G_REWARD_PROFITMAX_TRPENALTY_USERINCENTIVES 0 /* reward.py:34-44  */
#define EV2G_REWARD_SQUARED_TRACKING_ERROR 1             /* reward.py:7-14   */
#define EV2G_REWARD_PROFIT_MAXIMIZATION 2                /* reward.py:78-87  */
#define EV2G_REWARD_SQTR_TRPENALTY_USERINCENTIVES 3      /* reward.py:16-32: SqTrError_TrPenalty_UserIncentives        */
#define EV2G_REWARD_SQUARED_TRACKING_ERROR_PENALTY 4     /* reward.py:46-58: SquaredTrackingErrorRewardWithPenalty     */
#define EV2G_REWARD_SIMPLE 5                             /* reward.py:60-65: SimpleReward                              */
#define EV2G_REWARD_MINIMIZE_TRACKER_SURPLUS 6           /* reward.py:67-76: MinimizeTrackerSurplusWithChargeRewards   */
#define EV2G_REWARD_V2G_COSTS_SIMPLE 7                   /* reward.py:151-154: V2G_costs_simple                        */
#define EV2G_REWARD_V2G_PROFITMAX 8                      /* reward.py:120-148: V2G_profitmax                           */
#define EV2G_REWARD_V2G_PROFITMAX_V2 9                   /* reward.py:156-211: V2G_profitmaxV2                         */
#define EV2G_REWARD_PST_V2G_PROFITMAX_V2 10              /* reward.py:278-339: pst_V2G_profitmaxV2                     */
#define EV2G_N_REWARDS 11
/* Kinds 3, 8, 9 and 10 carry their own per-departure user term; the fused transformer_overload_usrpenalty cost (EV2G_COST_TR_OVERLOAD_
 * USRPENALTY) shares that staging slot and cannot be combined with them (ev2g_create refuses the pair).  The reference's other
 * reward built-ins need the grid simulation (V2G_grid_*) or are host-evaluated plugins through the Python facade. */
/* state_function built-ins (rl_agent/state.py) */
#define EV2G_STATE_V2G_PROFIT_MAX_LOADS 0 /* state.py:108-155, D = 2+H + 2H*R + 2P */
#define EV2G_STATE_PUBLIC_PST 1           /* state.py:6-63,    D = 3 + 3P          */
#define EV2G_STATE_V2G_PROFIT_MAX 2       /* state.py:65-106,  D = 2+H + 2P        */

/* cost_function built-ins (rl_agent/cost.py), evaluated next to the reward (ev2gym_env.py:434-438) */
#define EV2G_COST_NONE 0
#define EV2G_COST_TR_OVERLOAD_USRPENALTY 1 /* cost.py:8-18: 100*sum(overload) + 100*sum(exp(-10*score))  */
#define EV2G_COST_PROFIT_ONLY 2            /* cost.py:22-27 (ProfitMax_TrPenalty_UserIncentives_safety): total_costs */

#define EV2G_OK 0
#define EV2G_ERR_ARG -1       /* bad argument / inconsistent scenario                         */
#define EV2G_ERR_HIP -2       /* HIP runtime error                                            */
#define EV2G_ERR_STATE -3     /* call out of order (e.g. step before load)                    */
#define EV2G_ERR_DONE -4      /* step() after done: `assert not self.done` ev2gym_env.py:343  */
#define EV2G_ERR_OVERCURRENT -5 /* charger over-current Exception, ev_charger.py:203-205       */

#define EV2G_LUT_LEN 101 /* efficiency table 0..100 A, utils.py:282-288 */
#define EV2G_N_STATS 17  /* get_statistics() scalar keys, utils.py:84-101 */

/* flags for ev2g_config.flags */
#define EV2G_FLAG_LOG_CS_HISTORY 1 /* keep cs_power / cs_current [E,C,T] (ev2gym_env.py:533-535) */
#define EV2G_FLAG_NULL_STREAM 2    /* launch on the legacy default stream (torch's default stream) */
#define EV2G_FLAG_LOG_SOC 4        /* keep the per-step SoC log + |energy| sums that EV.get_battery_degradation needs
                                      (ev.py:156,162,180,185,442-521); without it the three degradation stats are NaN */
#define EV2G_FLAG_REFILLABLE 8     /* the resident scenario pool keeps a fixed-size block of session slots per scenario, so that
                                      ev2g_pool_refill can draw new scenarios into it ON THE DEVICE (default: packed storage)          */

typedef struct ev2g_handle ev2g_handle;

typedef struct ev2g_config {
    int32_t device;      /* HIP device ordinal                                                   */
    int32_t reward_kind; /* EV2G_REWARD_*  -- replaces the `reward_function` ctor kwarg (:47)    */
    int32_t state_kind;  /* EV2G_STATE_*   -- replaces the `state_function` ctor kwarg (:46)     */
    int32_t flags;       /* EV2G_FLAG_*                                                          */
    void *stream;        /* hipStream_t to launch on; NULL = a stream owned by the handle (or the
                            default stream with EV2G_FLAG_NULL_STREAM)                          */
    int32_t cost_kind;   /* EV2G_COST_*    -- replaces the `cost_function` ctor kwarg (:48)      */
    int32_t n_active_envs; /* E: envs stepped concurrently.  0 = as many as the loaded scenario pool holds.  With
                            E < pool size M the pool is a device-resident reservoir of scenarios and every reset
                            picks which M-cyclic window of it the E envs run (ev2g_reset_ex) -- the per-episode
                            scenario draw of EV2Gym.reset() (ev2gym_env.py:243-296) without a host round trip */
} ev2g_config;

/*
 * Scenario batch: every tensor EV2Gym.step() reads, for E independent envs that share one YAML
 * config (same chargers / sizes).  It is what the reference builds in __init__/reset()
 * (load_ev_charger_profiles loaders.py:299-365, load_transformers :227-296, EV_spawner
 * utils.py:477-557, load_electricity_prices loaders.py:392-461, load_power_setpoints :92-103).
 * HOST pointers, row-major, borrowed during the call.
 */
typedef struct ev2g_scenario_batch {
    int32_t n_envs;            /* E */
    int32_t n_steps;           /* T  = simulation_length                                  */
    int32_t timescale;         /* minutes per step                                        */
    int32_t n_chargers;        /* C                                                       */
    int32_t ports_per_charger; /* n_ports of every charger; with cs_n_ports: their maximum */
    int32_t n_transformers;    /* R                                                       */
    int32_t horizon;           /* H, must be 20                                           */
    int32_t n_dr_max;          /* ND: slots per transformer in tr_dr                      */
    int32_t n_lut;             /* NL efficiency tables                                    */
    int32_t reserved0;
    int64_t n_sessions;        /* total EV sessions over all envs = env_session_start[E]  */

    /* chargers [C]  (EV_Charger.__init__ ev_charger.py:41-94) */
    const double *cs_min_charge_current;
    const double *cs_max_charge_current;
    const double *cs_min_discharge_current; /* <= 0 */
    const double *cs_max_discharge_current; /* <= 0 */
    const double *cs_voltage;
    const int32_t *cs_phases;
    const int32_t *cs_transformer; /* connected_transformer, loaders.py:494-498 */
    /* n_ports of each charger when a topology file gives them different counts (loaders.py:312-340), or NULL: every
       charger has ports_per_charger ports.  Ports are numbered cumulatively in charger order (ev2gym_env.py:364-385). */
    const int32_t *cs_n_ports;

    /* per env [E,T]: row 0 of charge_prices / discharge_prices (identical for all chargers,
       loaders.py:423-424,439-442; charge price is negative) and power_setpoints */
    const double *charge_price;
    const double *discharge_price;
    const double *power_setpoints;

    /* per (env, transformer) [E,R,T]  (Transformer.__init__ transformer.py:38-78) */
    const double *tr_max_power;
    const double *tr_min_power;
    const double *tr_inflexible_load;
    const double *tr_solar_power;
    const double *tr_load_forecast; /* inflexible_load_forecast as it stands after reset() */
    const double *tr_pv_forecast;   /* pv_generation_forecast  as it stands after reset()  */
    const double *tr_dr;            /* [E,R,ND,3] (event_start_step, event_end_step, capacity_percentage) */
    const int32_t *tr_n_dr;         /* [E,R] number of valid events                        */
    const int32_t *tr_steps_ahead;  /* [E,R] transformer.py:66                             */

    /* EV sessions, CSR by env, in EVs_profiles order (sorted by arrival; utils.py:531-553) */
    const int64_t *env_session_start; /* [E+1] */
    const int32_t *ev_cs;             /* EV.location                                       */
    const int32_t *ev_t_arr;          /* time_of_arrival                                   */
    const int32_t *ev_t_dep;          /* time_of_departure                                 */
    const int32_t *ev_phases;         /* ev_phases                                         */
    const int32_t *ev_lut;            /* efficiency table id, -1 = scalar efficiencies     */
    const double *ev_cap0;            /* battery_capacity_at_arrival                       */
    const double *ev_B;               /* battery_capacity                                  */
    const double *ev_desired;         /* desired_capacity (kWh)                            */
    const double *ev_minB;            /* min_battery_capacity                              */
    const double *ev_min_emerg;       /* min_emergency_battery_capacity                    */
    const double *ev_pac_max;         /* max_ac_charge_power                               */
    const double *ev_pac_min;         /* min_ac_charge_power                               */
    const double *ev_pdis_max;        /* max_discharge_power (<= 0)                        */
    const double *ev_pdis_min;        /* min_discharge_power (<= 0)                        */
    const double *ev_ts;              /* transition_soc                                    */
    const double *ev_tsm;             /* transition_soc_multiplier                         */
    const double *ev_eta_ch;          /* scalar charge efficiency (ignored if ev_lut >= 0) */
    const double *ev_eta_dis;         /* scalar discharge efficiency                       */
    const double *lut;                /* [NL,101] percent, spawner fill utils.py:273-290   */
} ev2g_scenario_batch;

/* ---- lifetime ------------------------------------------------------------------------------ */
int ev2g_abi_version(void);
/* EV2Gym.__init__ (ev2gym_env.py:38-241): bind a device/stream and choose the fused hooks. */
int ev2g_create(const ev2g_config *cfg, ev2g_handle **out);
void ev2g_destroy(ev2g_handle *h);
const char *ev2g_last_error(const ev2g_handle *h); /* h may be NULL: last create() error */

/* The scenario-construction half of __init__/reset(): copies the batch to HBM, resolves every
 * session's port by replaying EV_Charger.spawn_ev's first-free rule (ev_charger.py:266-286,
 * action-independent), precomputes max_energy_AFAP (ev.py:407-440).  May be called again to
 * swap the scenario pool (same shapes or not).  Leaves the handle in the reset state. */
int ev2g_load_scenarios(ev2g_handle *h, const ev2g_scenario_batch *b);

/* shapes */
int ev2g_n_envs(const ev2g_handle *h);      /* E: envs stepped per call (n_active_envs)            */
int ev2g_n_scenarios(const ev2g_handle *h); /* M: scenarios resident in the pool (batch->n_envs)   */
int ev2g_n_ports(const ev2g_handle *h); /* P */
int ev2g_obs_dim(const ev2g_handle *h); /* D */
int ev2g_n_steps(const ev2g_handle *h); /* T */

/* ---- the hot path -------------------------------------------------------------------------- */
/* EV2Gym.reset() state-init part (ev2gym_env.py:298-306,329-331; init_statistic_variables
 * utils.py:794-861; EV_Charger.reset ev_charger.py:96-112) for every env of the batch, on the same
 * scenarios.  obs [E,D] may be NULL. */
int ev2g_reset(ev2g_handle *h, double *obs);
/* The same, preceded by the scenario draw of EV2Gym.reset() (ev2gym_env.py:243-296: new EV sessions, prices, loads,
 * PV, demand-response events, setpoints): env e runs scenario (e + scenario_offset) mod M of the resident pool for
 * the coming episode.  Distinct envs always run distinct scenarios (E <= M).  ev2g_reset() keeps the current offset
 * (re-arms the same scenarios); the host picks offsets (seeded, or fresh per episode).  O(1): nothing is copied. */
int ev2g_reset_ex(ev2g_handle *h, double *obs, int64_t scenario_offset);
int64_t ev2g_scenario_offset(const ev2g_handle *h);

/* EV2Gym.step(actions) for all E envs (ev2gym_env.py:333-447).
 *   actions     [E,P] float64, read-only here (the reference zeroes empty ports in the caller's
 *               array, ev_charger.py:139; the single-env Python facade reproduces that)
 *   obs         [E,D] state_function(env) after the step
 *   reward      [E]
 *   done        [E]   current_step >= simulation_length (:460)
 *   action_mask [E,P] 1 where a port holds an EV after the spawn phase (:452-457); may be NULL
 * Asynchronous on the handle's stream.  Returns EV2G_ERR_DONE if the batch is already done. */
int ev2g_step(ev2g_handle *h, const double *actions, double *obs, double *reward, uint8_t *done,
              uint8_t *action_mask);

/* K consecutive steps from a device-resident action source, enqueued without host round trips.
 * actions: [K,E,P] (action_step_stride = E*P) or one [E,P] block reused (stride 0).
 * Output k is written at base + k*<stride> elements.  Stride 0 = one buffer: after the call it holds the outputs of the
 * call's LAST step, every element of it written; what it holds while the steps run is unspecified (a persistent launch of
 * the specialised kernels -- ev2g_last_launch_specialisation 1, 2, 5 -- writes it in its last step only, the other paths
 * overwrite it step by step).  Pass step strides to keep the rows of every step.
 *   mode 0  one kernel launch per step, enqueued back to back from C;
 *   mode 1  ONE persistent launch: every workgroup loops over the K steps of its own envs (envs are
 *           independent, so no grid-wide synchronisation is needed).
 * If the episode ends inside the K steps: with auto_reset != 0 the envs are reset before the next step -- the
 * terminal step still reports its own obs -- otherwise stepping stops there and EV2G_ERR_DONE is returned.
 * auto_reset == 1 re-arms the same scenarios (ev2g_reset); auto_reset == 2 moves on to the next E scenarios of
 * the pool (ev2g_reset_ex with scenario_offset + E), inside the persistent launch as well -- as long as the windows
 * the run visits are disjoint ((resets + 1) * E <= M); a run whose windows overlap is issued as one persistent
 * launch per episode (results are identical: per-session results are indexed by pool scenario, and two envs must
 * not write one scenario's slots within a single launch). */
#define EV2G_AUTO_RESET_SAME 1
#define EV2G_AUTO_RESET_NEXT 2
#define EV2G_STEPN_PER_STEP_LAUNCH 0
#define EV2G_STEPN_PERSISTENT 1
int ev2g_step_n(ev2g_handle *h, int k_steps, int mode, const double *actions, int64_t action_step_stride,
                double *obs, int64_t obs_step_stride, double *reward, int64_t reward_step_stride,
                uint8_t *done, int64_t done_step_stride, uint8_t *action_mask,
                int64_t mask_step_stride, int auto_reset);

/* Optional extra step outputs / inputs, sticky until changed (all-NULL = off, the default).  DEVICE pointers.
 *   cost        [E] float64: cost_function value of the step (config.cost_kind must not be EV2G_COST_NONE)
 *   obs_f32     [E,D] float32 copy of the observation, written next to `obs` (which may then be NULL): policy
 *               networks take float32, this saves them a conversion pass over the largest stream of the path
 *   actions_f32 [E,P] float32 actions, read (and widened to float64 on entry, as every action is) when the
 *               `actions` argument of ev2g_step / ev2g_step_n is NULL; its step stride is action_step_stride */
typedef struct ev2g_step_extras {
    double *cost;
    int64_t cost_step_stride;
    float *obs_f32;
    int64_t obs_f32_step_stride;
    const float *actions_f32;
} ev2g_step_extras;
int ev2g_set_step_extras(ev2g_handle *h, const ev2g_step_extras *x); /* x == NULL clears */

int ev2g_current_step(const ev2g_handle *h);
/* Which step kernel ev2g_load_scenarios selected for the loaded shape ("ev2g_step_wave<0,0>", "ev2g_step_v2<1024>",
 * "ev2g_step_kernel"), and -- when the common-shape fast path was not taken -- why ("" otherwise). */
const char *ev2g_kernel_name(const ev2g_handle *h);
const char *ev2g_fallback_reason(const ev2g_handle *h);
/* Round 6: big envs (512 < ports <= 1024) loaded on "ev2g_step_v2<1024>" run their specialised launches (ev2g_last_launch_specialisation 5) on
 * "ev2g_step_big" when the batch qualifies; this returns why it does NOT ("" when it does, or when the shape is not a big env). */
const char *ev2g_big_kernel_reason(const ev2g_handle *h);
/* Which instantiation of the fast-path kernel the last ev2g_step / ev2g_step_n launch used: 0 = the general one (any subset of outputs,
 * strides, extras, in-launch resets); 1 = "full" (all four outputs with step stride 0 -- float64 actions in and float64 observations out, or, with the float32 action and
 * observation buffers of ev2g_set_step_extras registered and no float64 ones passed, float32 in and out: ev2g_rollout --, no cost output, no charger
 * histories, the launch ends within the episode, one of the three compiled-in rewards): their checks are compiled out; 2 = full, plus
 * EV2G_FLAG_LOG_SOC on and an env wide enough for one observation-head column pair per lane.  The general kernel ("ev2g_step_v2<..>") has
 * one such instantiation (1) for the reference's default plugin pair -- V2G_profit_max_loads + ProfitMax_TrPenalty_UserIncentives, single-port
 * chargers, everything of the float64 list above, EV2G_FLAG_LOG_SOC, 15 / 30 / 60-minute steps -- and 0 otherwise.  -1: no launch yet, or the
 * generic kernel.
 * Round 5: 3 = 2 for outputs with STEP STRIDES (float64 [K,E,*] observation / reward / done / mask blocks of a persistent launch, every step kept:
 * generate_trajectories.py:69-83 style use; needs what 2 needs); 4 = the fused actor + step launch of ev2g_rollout / ev2g_collect (the policy
 * evaluated inside the step kernel's launch, one launch per segment; below).
 * Round 6: 5 = big envs (512 < ports <= 1024, single-port chargers, <= 50 transformers, <= 16 distinct charger tuples, windows below 16384 steps):
 * what 1 covers is run by "ev2g_step_big" -- 512 threads, two ports per home lane, 70 bytes of LDS per port, TWO workgroups per CU.  Port state,
 * observations, masks and transformer powers are bit-identical to 0 / 1; rewards and the episode sums of profits / energies come from a different
 * fixed summation tree (last-bit differences, tests hold them to 1e-12).  EV2G_NO_BIG=1 at load time keeps 1.
 * Results are identical in all of them (tests/test_round3_gpu.py, test_round4_gpu.py, test_round5_gpu.py); EV2G_NO_FULL / EV2G_NO_WIDE /
 * EV2G_NO_STRIDED in the environment at load time force 0 / 1 / "strided outputs run 0"; EV2G_NO_DICT=1 at load time keeps the battery-maths operands
 * one record per session instead of in the per-model dictionary, EV2G_NO_FUSED=1 keeps ev2g_rollout / ev2g_collect at two launches per step
 * (EV2G_NO_FUSED_F32=1: only the float32 policy). */
int ev2g_last_launch_specialisation(const ev2g_handle *h);
/* When the last fast-path launch got the general instantiation (0): what the caller passed or configured that ruled the full one out (the
 * first such thing), "" otherwise.  The Python Engine warns once with it: the general instantiation is ~20 % slower, silently. */
const char *ev2g_last_launch_general_reason(const ev2g_handle *h);
/* Where the last ev2g_get_stats / ev2g_get_stats_reset took the statistics from: 1 = computed inside the step launch that closed the episode
 * (a launch of specialisation 2 ending at the last step, one env per wavefront: its workgroups compute their envs' statistics once they
 * have stepped them) and copied -- ev2g_get_stats_reset is then a reset-only launch that also copies the rows; 0 = computed by the
 * statistics kernel (a mid-episode call, per-step launches, the other instantiations and kernels, or EV2G_NO_INLAUNCH_STATS=1 at load time);
 * -1 = no such call yet.  The values are bit-identical either way.  Any state-changing call (step, reset, refill, load) discards the in-launch
 * results. */
int ev2g_last_stats_route(const ev2g_handle *h);
/* When ev2g_last_stats_route is 0: why the in-launch statistics were not available, "" otherwise. */
const char *ev2g_last_stats_reason(const ev2g_handle *h);
/* Fast-forwarded EV-free stretches.  A persistent launch (k > 1) of the stride-0 float64 specialisations (ev2g_last_launch_specialisation 1 or 2) with
 * one env per wavefront (33..64 ports) and a head-table state (V2G_profit_max, V2G_profit_max_loads; not PublicPST) does not step a stretch of steps in which none of a workgroup's four envs holds an EV or receives one: it
 * writes those steps' history rows and adds their rewards to the episode return in one pass, up to but never including the launch's last step.
 * `hist`, the accumulators and everything derived from them (the statistics) are bit-identical to stepping those steps one by one.
 * This call reports what the LAST launch skipped that way, summed over its workgroups: workgroup-steps, and stretches counted as passes of at most 64
 * steps each (either pointer may be NULL).
 * Both are 0 after any launch that is not eligible (other instantiations and kernels, single steps, several envs per wavefront) and when the
 * library was loaded with EV2G_NO_FAST_FORWARD=1, which steps every step (A/B runs, parity tests).  Synchronises the stream. */
int ev2g_last_launch_fast_forwarded(ev2g_handle *h, int64_t *steps, int64_t *stretches);
/* CU balance.  The launches that fast-forward (above) are as long as their busiest compute unit, and a live step costs more the more workgroups
 * its CU still holds.  Such a launch that starts at step 0 is therefore handed a map workgroup -> env group that deals the groups of the pool window
 * it steps, heaviest first (most steps with an EV present or arriving: a function of the scenarios, not of the actions), over the CUs as a snake,
 * so that every CU's workgroups have about the same work in sum.  A map is a permutation of the groups and all state is indexed by env: results
 * are bit-identical with and without it.  A window's map is made once (at load for the offsets k * n_envs, else at the first launch on it) and
 * kept on the device.  Not for episodes of more than 256 steps or EV2G_FLAG_REFILLABLE handles; EV2G_NO_CU_BALANCE=1 at load time switches it off.
 * Returns 1 when the LAST step launch had a map (`moved`: the workgroups that stepped another group than without one), else 0 and `reason` says why
 * (either pointer may be NULL; the string lives as long as the handle). */
int ev2g_last_launch_balance(const ev2g_handle *h, int64_t *moved, const char **reason);
/* Development: where the workgroups of the LAST launch ran.  Only a library loaded with EV2G_PLACEMENT=1 records it, and only in the launches that
 * fast-forward (above); such a launch is preceded by a memset on the stream and every workgroup does one atomic addition, so do not time with it.
 * Two words per workgroup b = blockIdx.x: out[2 b] = HW_REG_XCC_ID << 16 | the low 16 bits of HW_REG_HW_ID (bits 8..15: CU, SH, SE), out[2 b + 1] =
 * how many workgroups of the launch had arrived on that CU before it.  Returns the number of workgroups written (`n_words` must hold twice as many),
 * 0 when nothing was recorded, or an error code (< 0).  Synchronises the stream. */
int ev2g_last_launch_placement(ev2g_handle *h, uint32_t *out, int64_t n_words);
/* data-dependent faults recorded since the last reset (per-env flag word, device side):
 * returns 0 or EV2G_ERR_OVERCURRENT; synchronises the stream. */
int ev2g_check_faults(ev2g_handle *h, int32_t *first_bad_env);

/* ---- episode statistics (get_statistics utils.py:12-123) ------------------------------------ */
/* stats [E,EV2G_N_STATS] float64 DEVICE pointer, key order = ev2g_stat_name(i). */
int ev2g_get_stats(ev2g_handle *h, double *stats);
/* ev2g_get_stats followed by ev2g_reset_ex(h, obs, scenario_offset) in ONE kernel launch: what an auto-resetting vectorised env does at an
 * episode end (terminal info = get_statistics(), then reset(); ev2gym_env.py:243-331 + utils.py:12-123).  The wavefront that computed an env's
 * statistics re-arms that env on the new pool window; `obs` (DEVICE, may be NULL) receives the reset observation like ev2g_reset_ex. */
int ev2g_get_stats_reset(ev2g_handle *h, double *stats, double *obs, int64_t scenario_offset);
/* The same with the reset observation as float32 (the policy-network side of ev2g_collect / ev2g_rollout), and the plain reset with a float32
 * observation: `obs32` DEVICE [E, D] or NULL. */
int ev2g_get_stats_reset_f32(ev2g_handle *h, double *stats, float *obs32, int64_t scenario_offset);
int ev2g_reset_f32(ev2g_handle *h, float *obs32, int64_t scenario_offset);
const char *ev2g_stat_name(int i);

/* ---- multi-GPU: one process per GPU, envs sharded, statistics gathered over RCCL ---------------
 * The reference has no multi-process path (one env, one process).  Sharding envs over GPUs needs no data-path collective;
 * the only exchange is this per-episode statistics block.  For hosts without torch.distributed: rank 0 obtains an id,
 * ships its EV2G_COMM_ID_BYTES bytes to the other ranks by any host-side means, every rank calls ev2g_comm_init, and
 * ev2g_gather_stats then computes this rank's statistics and all-gathers them with ncclAllGather on the handle's stream
 * (stream-ordered, asynchronous to the host).  Every rank must hold the same number of envs.  librccl is opened on first
 * use; without it these calls fail with EV2G_ERR_STATE and the step path is unaffected. */
#define EV2G_COMM_ID_BYTES 128
int ev2g_comm_get_unique_id(void *id_out);
int ev2g_comm_init(ev2g_handle *h, const void *id, int rank, int world_size);
void ev2g_comm_destroy(ev2g_handle *h);
int ev2g_comm_world_size(const ev2g_handle *h);   /* 0: no communicator */
long long ev2g_comm_gathers(const ev2g_handle *h); /* all-gathers issued so far */
/* stats_all: DEVICE [world_size * E, EV2G_N_STATS] float64, rank-major */
int ev2g_gather_stats(ev2g_handle *h, double *stats_all);

/* ---- inspection (feeds the read-only Python facade of the reference object graph) ----------- */
/* HOST output buffers; any may be NULL.  Synchronises.  Port arrays are in reference port order;
 * empty ports are NaN / -1.  */
typedef struct ev2g_env_view {
    int32_t current_step;
    int32_t n_ports, n_chargers, n_transformers, n_steps;
    double *port_capacity;        /* [P] EV.current_capacity                */
    double *port_energy;          /* [P] EV.current_energy                  */
    double *port_current;         /* [P] EV.actual_current                  */
    double *port_total_energy;    /* [P] EV.total_energy_exchanged          */
    double *port_required_energy; /* [P] EV.required_energy                 */
    double *port_prev_power;      /* [P] EV.previous_power                  */
    int32_t *port_cycles;         /* [P] EV.charging_cycles                 */
    int32_t *port_session;        /* [P] index into the env's session list  */
    double *cs_power;             /* [C] EV_Charger.current_power_output    */
    double *cs_amps;              /* [C] EV_Charger.current_total_amps      */
    double *cs_profits;           /* [C] total_profits                      */
    double *cs_energy_charged;    /* [C] total_energy_charged               */
    double *cs_energy_discharged; /* [C] total_energy_discharged            */
    double *tr_power;             /* [R] Transformer.current_power          */
    double *tr_overload;          /* [R,T] env.tr_overload                  (the three histories: entries of steps the running episode has   */
    double *power_usage;          /* [T] env.current_power_usage             not reached yet are zeros, like the reference's arrays, whatever  */
    double *power_potential;      /* [T] env.charge_power_potential          an earlier episode left in the device buffers)                   */
    int32_t *session_port;        /* [S_env] resolved port of every session */
    double *session_afap;         /* [S_env] EV.max_energy_AFAP             */
    double *session_final_cap;    /* [S_env] capacity at departure (NaN while not departed) */
} ev2g_env_view;
int ev2g_peek(ev2g_handle *h, int env, ev2g_env_view *view);

/* ---- policy in the loop (BASELINE configs[4]: an SB3-MlpPolicy-shaped actor produces the actions between steps) ------ */
/* A three-layer MLP actor  obs[E,d_in] -> ReLU(h1) -> ReLU(h2) -> tanh(d_out)  evaluated by ONE kernel (bf16 MFMA, fp32
 * accumulation).  Weights are HOST pointers in torch.nn.Linear layout (W[out,in] row-major, b[out]), copied and packed once.
 * out_lo = -1: actions in [-1,1] (tanh); out_lo = 0: (tanh + 1) / 2, the action box of configs without V2G (ev2gym_env.py:226-231).
 * The reference has no counterpart: its agents are SB3 objects stepping one CPU env (train_stable_baselines.py:62-130). */
typedef struct ev2g_mlp ev2g_mlp;
int ev2g_mlp_create(ev2g_handle *h, int d_in, int h1, int h2, int d_out, const float *W1, const float *b1, const float *W2,
                    const float *b2, const float *W3, const float *b3, float out_lo, ev2g_mlp **out);
/* The same with the operand precision chosen, for policies trained in float32 (SB3's are):
 *   EV2G_MLP_BF16   (the call above) weights and activations rounded to bf16: fastest, actions within ~1e-2 of a float32 forward;
 *   EV2G_MLP_F32    float32 weights held as TWO bf16 terms (16 significant bits), activations as three, five MFMA products per k-step: the
 *                   device forward agrees with a float64 forward of the same weights to 1e-5 (observed 4e-6), at twice the bf16 time;
 *   EV2G_MLP_F32X3  three terms per weight (all 24 bits), six products: agreement at the 1e-7 level -- what float32 operands give --
 *                   at 2.6x the bf16 time.
 * Networks that fit the shipped shapes (inputs <= 192, hidden layers <= 400 / 304 with at least one >= 128, outputs <= 64) run all three modes on
 * the same streaming kernel on the bf16 matrix cores, zero-padded where they are smaller (the weight stream is the cost: 1x, 2x, 3x the bytes);
 * other networks fall back to generic kernels (bf16, and float32 operands on v_mfma_f32_32x32x2_f32 for both float32 modes). */
#define EV2G_MLP_BF16 0
#define EV2G_MLP_F32 1
#define EV2G_MLP_F32X3 2
int ev2g_mlp_create_ex(ev2g_handle *h, int d_in, int h1, int h2, int d_out, const float *W1, const float *b1, const float *W2,
                    const float *b2, const float *W3, const float *b3, float out_lo, int precision, ev2g_mlp **out);
/* Which actor kernel the policy got (csrc/ev2g_policy_host.h: plan_mlp), as the instantiation's name: "ev2g_mlp3_any", "ev2g_mlp3_f32",
 * "ev2g_mlp3_fixed<11,26,20>", "ev2g_mlp3_s16<6,25,19,4,1,8>" (the streaming kernel: k-steps of layer 1, 16-column tiles of the three layers,
 * bf16 terms per weight, wavefronts per workgroup).  A bf16 streaming policy runs large batches on the 32-row variant; the string then goes on
 * with "; from <rows> rows <that instantiation>", e.g. "ev2g_mlp3_s16<6,25,19,4,1,8>; from 4097 rows ev2g_mlp3_s16<6,25,19,4,1,4,2>".
 * Owned by the policy, valid until ev2g_mlp_destroy; "" for NULL. */
const char *ev2g_mlp_kernel_name(const ev2g_mlp *m);
void ev2g_mlp_destroy(ev2g_handle *h, ev2g_mlp *m);
/* y[n_rows,d_out] = actor(x[n_rows,d_in]); float32 DEVICE pointers; asynchronous on the handle's stream. */
int ev2g_mlp_forward(ev2g_handle *h, const ev2g_mlp *m, const float *x, float *y, int n_rows);
/* K rollout steps enqueued by one call: actor(obs_f32) -> actions_f32 -> EV2Gym.step, K times (the float32 buffers are the ones
 * registered with ev2g_set_step_extras, obs_f32_step_stride 0; d_in == obs dim, d_out == ports).  reward / done /
 * action_mask as in ev2g_step_n (mode EV2G_STEPN_PER_STEP_LAUNCH); auto_reset as there.
 * Round 5: ONE launch per segment where the shape is eligible -- the fast path (3..64 ports per env: the shipped V2GProfitPlusLoads
 * file's 25 chargers, BASELINE's 50), a V2G_profit_max(_loads) state, a compiled-in reward, EV2G_FLAG_LOG_SOC, no cost buffer, all three outputs
 * present, the segment inside the episode, and the bf16 policy in the 162 -> 400 -> 300 -> 64 packing: the workgroup that steps 16 envs
 * evaluates the policy on their 16 observation rows between the steps (same MFMA chains as ev2g_mlp_forward: bit-identical actions), so
 * neither kernel pays a cold start per step and the port state stays in LDS across the segment.  Anything else runs actor and step as two
 * launches per step, as before (train_stable_baselines.py:62-130 is the loop this replaces).
 * Round 6: PublicPST too (two envs per wavefront), and the FLOAT32 policy (EV2G_MLP_F32; one env per wavefront for every state): the same five-product chain per
 * k-step as ev2g_mlp_forward's (bit-identical actions), input rows kept float32 in LDS and split into their three bf16 terms where they are read;
 * EV2G_NO_FUSED_F32=1 keeps that policy at two launches per step.  EV2G_MLP_F32X3 policies always run two launches per step. */
int ev2g_rollout(ev2g_handle *h, const ev2g_mlp *m, int k_steps, double *reward, int64_t reward_step_stride, uint8_t *done,
                 int64_t done_step_stride, uint8_t *action_mask, int64_t mask_step_stride, int auto_reset);
/* Segments that contain no episode end are captured once as a HIP graph (keyed by their full launch signature) and replayed;
 * EV2G_ROLLOUT_GRAPHS=0 in the environment falls back to plain launches.  Number of graph replays so far: */
long long ev2g_rollout_graph_launches(const ev2g_handle *h);

/* Off-policy ROLLOUT COLLECTION into device memory (the collect_rollouts() half of an SB3 DDPG / TD3 loop,
 * train_stable_baselines.py:62-130; SAC's, with its stochastic actor, is ev2g_sac_collect over the same arrays): k_steps x (actor forward -> env step) whose transitions land directly in the caller's device arrays --
 * no host copy, no staging copy: the actor reads observation row i and writes action row i, the step kernel reads that action row and writes
 * observation row i + 1, reward / done / mask row i.  With next_obs[i] = obs[i + 1] these arrays ARE a replay-buffer segment (SB3's
 * ReplayBuffer(optimize_memory_usage=True) layout).  obs[0] is input: the observation the first action is computed from (the reset
 * observation, or the last row of the previous segment).  The segment must end at or before the episode end; statistics, the reset and
 * the terminal observation (= the segment's last observation row) are the caller's (ev2g_get_stats_reset).  All pointers DEVICE.
 * Eligible shapes run the whole segment as ONE fused launch (see ev2g_rollout); rows and values are the same either way. */
typedef struct {
    float *obs;         /* [k_steps + 1, E, D]; row 0 read, rows 1.. written */
    float *actions;     /* [k_steps, E, P] written */
    double *reward;     /* [k_steps, E] written */
    uint8_t *done;      /* [k_steps, E] written */
    uint8_t *mask;      /* [k_steps, E, P] written */
} ev2g_transitions;
int ev2g_collect(ev2g_handle *h, const ev2g_mlp *m, int k_steps, const ev2g_transitions *tr);

/* ---- the reference's env-reading heuristic agents ON THE DEVICE (baselines/heuristics.py) ----------------------------------------------
 * The agent reads the engine's state before each step -- which ports hold an EV, its capacity, departure, desired capacity, the step's power
 * setpoint -- and writes float64 actions [E,P] in the reference's port order, bit for bit what the reference's agent chooses on that env
 * (same operation order).  The RoundRobin agents keep their queue of ports per env on the device; it is emptied at step 0 of every episode, like the
 * fresh agent the reference's evaluator builds for every run (evaluator.py:237). */
#define EV2G_HEURISTIC_CHARGE_AS_LATE_AS_POSSIBLE 0         /* heuristics.py:98-149  */
#define EV2G_HEURISTIC_CHARGE_AS_FAST_TO_DESIRED_CAPACITY 1 /* heuristics.py:230-267 */
#define EV2G_HEURISTIC_ROUND_ROBIN 2                        /* heuristics.py:7-96    */
/* Three more kinds in the SAME number space (ev2g_heuristic_create's `kind`).  They carry another prefix because the EV2G_HEURISTIC_* list
 * is a frozen set that existing callers and checks enumerate; the union of both lists is what _abi.AGENT_KINDS mirrors.
 *  - the two RoundRobin_GF agents keep, next to their queue of ports, the min_power / max_power every queue entry was INSERTED with, as the
 *    reference does: a port whose next EV arrives the step after the last one left stays queued with the old EV's powers;
 *  - they exist for one-port chargers only: the reference indexes its per-charger power table with a port id and divides by zero otherwise, so
 *    ev2g_heuristic_create returns EV2G_ERR_ARG for them when any charger of the loaded scenarios has more than one port, and so do
 *    ev2g_heuristic_actions / _run for a live agent after a reload brought such chargers;
 *  - their selection is a sequential float64 sum in queue order: a plain left-to-right sum from 0, which is what the reference's sum()
 *    computes under CPython before 3.12 (from 3.12 on sum() compensates float sums and the reference itself gives other bits);
 *  - at most 3100 ports per env (RoundRobin: 13000), refused at create. */
#define EV2G_AGENT_CHARGE_AS_LATE_TO_DESIRED_CAPACITY 3     /* heuristics.py:561-622 */
#define EV2G_AGENT_ROUND_ROBIN_GF 4                         /* heuristics.py:270-399 */
#define EV2G_AGENT_ROUND_ROBIN_GF_OFF_ALLOWED 5             /* heuristics.py:402-530 */
typedef struct ev2g_heuristic ev2g_heuristic;
/* needs loaded scenarios; the agent is bound to the handle's env and port counts (a reload that changes them makes its calls fail) and is
 * freed with the handle if not before */
int ev2g_heuristic_create(ev2g_handle *h, int kind, ev2g_heuristic **out);
void ev2g_heuristic_destroy(ev2g_handle *h, ev2g_heuristic *a);
/* the agent's actions for the current step into actions [E,P] (DEVICE); no step is taken.  A RoundRobin agent's queue advances as in get_action(). */
int ev2g_heuristic_actions(ev2g_handle *h, ev2g_heuristic *a, double *actions);
/* k_steps x (agent -> one step) inside ONE episode, enqueued without host round trips: the agent's launch, then a one-step launch of the step
 * kernel the handle selected.  actions [k,E,P] written at base + k*a_stride (NULL: a buffer of the agent, stride 0); obs / reward / done /
 * mask as in ev2g_step_n (DEVICE, each may be NULL).  A segment that would run past the episode end returns EV2G_ERR_DONE: reset in between
 * (with auto-reset the engine re-arms an env inside the next step launch, after the agent would have read it).  Timed like ev2g_step_n
 * (ev2g_last_step_n_kernel_ms). */
int ev2g_heuristic_run(ev2g_handle *h, ev2g_heuristic *a, int k_steps, double *actions, int64_t a_stride, double *obs, int64_t o_stride,
                       double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride);

/* ---- the reference's communication-fault models ON THE DEVICE (rl_agent/noise_wrappers.py) ------------------------------------------------
 * A link holds both of the reference's robustness wrappers for the E envs of a handle:
 *   FailedActionCommunication (noise_wrappers.py:12-60): a charger whose uniform of the step is below p_fail keeps executing the command it
 *     was sent last (zeros before the first); what is held is what was SENT, not what the env left of it after zeroing empty ports;
 *   DelayedObservation (noise_wrappers.py:62-198, the PublicPST branch): an occupied slot whose uniform of the step is below p_delay shows the
 *     energy column delivered one step earlier, and the power reading obs[2] is lowered by the energy that was not communicated,
 *     (nc * 60) / timescale, nc summed over the delayed slots in slot order (a plain left-to-right float64 sum), and clamped at 0 last.
 * Both are bit for bit the reference's arithmetic.  Like the reference's objects a link keeps its uniforms and its held commands / remembered
 * rows ACROSS episodes (ev2g_link_reset_state zeroes the latter: the fresh wrapper a caller builds per run, evaluator.py:237 style).
 * Uniforms of each half: a HOST matrix in the reference's layout [E,P,T] (env e's [P,T] matrix is the wrapper's `random`; row i pairs with
 * port / observation slot i), uploaded once -- or NULL: the counter-based generator of ev2g_fill_uniform evaluated on the fly at index
 * (e*P + i)*T + t under the half's seed, i.e. the matrix ev2g_host_uniform(., E*P*T, seed, 0, 1) fills, without allocating it.
 * Two stated differences to the reference:
 *  - at the terminal observation (current_step == T) the reference indexes random[:, T] and raises as soon as one port is occupied; here that
 *    observation passes through with no slot delayed (nc = 0, remembered rows updated, clamp applied);
 *  - the reference's `assert obs[2] >= -5` (noise_wrappers.py:193) is not reproduced, only the clamp.
 * Out of scope: the wrapper's graph-state branch (noise_wrappers.py:134-161); the action wrappers (rl_agent/action_wrappers.py) are ev2g_wrap_* below. */
typedef struct ev2g_link ev2g_link;
/* Needs loaded scenarios; bound to the handle's envs, ports and steps like an agent (a reload that changes them makes its calls fail) and freed
 * with the handle if not before.  EV2G_ERR_ARG: a probability outside [0,1]; p_delay > 0 on a handle whose state is not EV2G_STATE_PUBLIC_PST
 * (noise_wrappers.py:79-80).  A probability of exactly 0 disables that half: ev2g_link_run launches nothing for it (its matrix is not uploaded). */
int ev2g_link_create(ev2g_handle *h, double p_fail, double p_delay, uint64_t seed_act, uint64_t seed_obs, const double *rand_act,
                     const double *rand_obs, ev2g_link **out);
void ev2g_link_destroy(ev2g_handle *h, ev2g_link *l);
/* zeroes the held commands and the remembered rows (noise_wrappers.py:32,105-106: a freshly constructed pair of wrappers) */
int ev2g_link_reset_state(ev2g_handle *h, ev2g_link *l);
/* FailedActionCommunication.action (noise_wrappers.py:37-60) for step t (t < 0: the handle's current step): `in` [E,P] DEVICE, float64 or --
 * in_is_f32 != 0 -- float32, widened as the engine widens float32 actions; the delivered commands go to the link (they are the next call's
 * previous ones) and to out [E,P] float64 (DEVICE, may be NULL).  No step is taken.  EV2G_ERR_DONE for t >= T. */
int ev2g_link_actions(ev2g_handle *h, ev2g_link *l, int t, const void *in, int in_is_f32, double *out);
/* DelayedObservation.observation (noise_wrappers.py:113-198) on the observation of step t (t < 0: the handle's current step; 0 = the reset
 * observation, T = the terminal one, which passes through): obs [E,D] DEVICE is rewritten in place; obs32 [E,D] (DEVICE, may be NULL) receives
 * the delivered row rounded to float32.  PublicPST handles only. */
int ev2g_link_observe(ev2g_handle *h, ev2g_link *l, int t, double *obs, float *obs32);
/* k_steps x ([agent ->] fail kernel -> one-step launch of the step kernel the handle selected -> delay kernel on the observation row it wrote)
 * inside ONE episode, enqueued without host round trips.  agent == NULL: the raw actions are read from actions [k,E,P] (a_stride 0: one block
 * reused); with an agent (ev2g_heuristic_create) its raw actions are written there when it is not NULL.  obs / reward / done / mask as in
 * ev2g_step_n (DEVICE, each may be NULL; the delayed half then works on a row of the link).  obs holds the DELIVERED observations.  A segment
 * that would run past the episode end returns EV2G_ERR_DONE, as ev2g_heuristic_run does.  Timed like ev2g_step_n (ev2g_last_step_n_kernel_ms).
 * A link that delays (p_delay > 0) must be shown every episode's RESET observation first, as the reference's wrapper is (noise_wrappers.py:113
 * on reset): ev2g_reset into a block, then ev2g_link_observe(h, l, 0, that block, NULL), before the first segment.  Without it the remembered
 * rows still hold the previous episode's terminal observation (zeros on a fresh link) when step 1's observation is delayed. */
int ev2g_link_run(ev2g_handle *h, ev2g_link *l, ev2g_heuristic *agent, int k_steps, double *actions, int64_t a_stride, double *obs,
                  int64_t o_stride, double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride);
/* The policy loop under the link: k_steps x (ev2g_mlp_forward on the link's float32 delivered row -> fail kernel on the policy's float32
 * actions -> one-step launch -> delay kernel writing the float64 row and its float32 copy), inside one episode.  The rows live in the link;
 * ev2g_link_obs_f32 returns the float32 one [E,D] (DEVICE): fill it before the first segment of an episode, with ev2g_link_observe(h, l, 0,
 * reset observation, that pointer) -- or ev2g_reset_f32 into it for a link that delays nothing.  The unfused chain only: there is NO
 * fused-launch variant (ev2g_rollout's single launch per segment has no place for the two kernels between policy and step). */
float *ev2g_link_obs_f32(ev2g_handle *h, ev2g_link *l);
int ev2g_link_rollout(ev2g_handle *h, ev2g_link *l, const ev2g_mlp *m, int k_steps, double *reward, int64_t r_stride, uint8_t *done,
                      int64_t d_stride, uint8_t *mask, int64_t m_stride);

/* ---- the reference's action wrappers ON THE DEVICE (rl_agent/action_wrappers.py) -------------------------------------------------------------
 * A wrapper rewrites the raw actions [E,P] of the current step into the actions the step reads, for the E envs of a handle, in float64 and in
 * the reference's operation order (bit for bit its arithmetic).  min_action[p] = cs_min_charge_current / cs_max_charge_current + 1e-4 of
 * port p's charger.
 *   EV2G_WRAP_BINARY          BinaryAction (action_wrappers.py:47): in > 0.5 ? 1 : min_action[p];
 *   EV2G_WRAP_THREE_STEP      ThreeStep_Action and ThreeStep_Action_DiscreteActionSpace (:90, :138): in == 0 ? 0 : (in == 1 ? min_action[p] : 1);
 *   EV2G_WRAP_RESCALE_REPAIR  Rescale_RepairLayer (:277-451): a = in * (1 - min_action) + min_action; the wrapper's queue of ports whose EV is
 *     below full charge is updated (update_ev_buffer, :205-243); the queued EVs' clamped powers are raised proportionally towards the step's
 *     power setpoint, or reduced proportionally and then topped up greedily in queue order, or left alone when they meet it exactly; the
 *     result is a[p] * occupied_ports[p].  Every sum is the plain left-to-right float64 sum in queue order (Python's sum() before CPython
 *     3.12).  One port per charger only (:186).  The queue lives in the wrapper ACROSS episodes, as the reference's object does
 *     (ev2g_wrap_reset_state empties it: a freshly built wrapper).  Two quirks of the reference are reproduced:
 *      - a queue entry keeps the min_power / max_power it was inserted with: a port whose next EV arrives the step after the last one left
 *        stays queued with the old EV's powers;
 *      - new_action[i] = proposed_power[i] / max_cs_power[i] divides by the charger at the QUEUE POSITION i, not by the entry's own port
 *        (:356, :429); with chargers of unequal power the two differ.
 * The discretisers work for any number of ports per charger.  MinMax_RepairLayer raises in the reference's constructor and has no kind; mask_fn
 * is left out.  A step chain holds a wrapper OR a link / grid, not both; stacked wrappers are not supported. */
#define EV2G_WRAP_BINARY 0
#define EV2G_WRAP_THREE_STEP 1
#define EV2G_WRAP_RESCALE_REPAIR 2
typedef struct ev2g_wrap ev2g_wrap;
/* Needs loaded scenarios; bound to the handle's envs and ports like an agent (a reload that changes them makes its calls fail) and freed with
 * the handle if not before.  EV2G_ERR_ARG: an unknown kind; EV2G_WRAP_RESCALE_REPAIR on chargers with several ports, or above 2259 ports per
 * env (one env's queue stage has to fit the 64 KiB of LDS). */
int ev2g_wrap_create(ev2g_handle *h, int kind, ev2g_wrap **out);
void ev2g_wrap_destroy(ev2g_handle *h, ev2g_wrap *w);
/* empties the repair layer's queue of every env (a freshly constructed wrapper); nothing to do for the discretisers */
int ev2g_wrap_reset_state(ev2g_handle *h, ev2g_wrap *w);
/* The wrapper's action() for the handle's current step: `in` [E,P] DEVICE, float64 or -- in_is_f32 != 0 -- float32, widened as the engine widens
 * float32 actions; out [E,P] float64 DEVICE, which may be a float64 `in` (rewritten in place).  No step is taken; the repair layer's queue
 * advances as the reference's does on every action() call.  EV2G_ERR_DONE past the episode's last step. */
int ev2g_wrap_actions(ev2g_handle *h, ev2g_wrap *w, const void *in, int in_is_f32, double *out);
/* k_steps x (wrapper kernel -> one-step launch of the step kernel the handle selected) inside ONE episode, enqueued without host round trips.
 * The raw actions are read from actions [k,E,P] at base + k*a_stride (a_stride 0: one block reused); the wrapped actions are written to
 * wrapped [k,E,P] at base + k*w_stride (NULL: a block of the wrapper, stride 0), which the step reads.  obs / reward / done / mask as in
 * ev2g_step_n (DEVICE, each may be NULL).  A segment that would run past the episode end returns EV2G_ERR_DONE, as ev2g_heuristic_run does.
 * Timed like ev2g_step_n (ev2g_last_step_n_kernel_ms). */
int ev2g_wrap_run(ev2g_handle *h, ev2g_wrap *w, int k_steps, double *actions, int64_t a_stride, double *wrapped, int64_t w_stride, double *obs,
                  int64_t o_stride, double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride);
/* The policy loop under a wrapper: k_steps x (ev2g_mlp_forward between the float32 buffers registered with ev2g_set_step_extras -> wrapper
 * kernel on the policy's float32 actions -> one-step launch reading the wrapper's float64 block and writing the float32 observation), inside
 * one episode: ev2g_rollout's two-launch chain plus one launch, unfused and not captured into a graph.  EV2G_ERR_ARG for EV2G_WRAP_THREE_STEP
 * (a tanh output never equals 0 or 1), without the registered pair, or unless the actor maps D -> P. */
int ev2g_wrap_rollout(ev2g_handle *h, ev2g_wrap *w, const ev2g_mlp *m, int k_steps, double *reward, int64_t r_stride, uint8_t *done,
                      int64_t d_stride, uint8_t *mask, int64_t m_stride);

/* ---- the distribution grid's power flow ON THE DEVICE (simulate_grid: models/grid.py, models/grid_utility/grid_tensor.py) ----------------
 * A grid holds the reference's Laurent power flow (pf_solver "Laurent", constant-power loads) for the E envs of a handle.  After every step
 * the reference injects each transformer's current_power at its bus (ev2gym_env.py:387-393: node i + 1 <- transformer i), adds the step's base
 * load minus PV (grid.py:110-139), and iterates from a flat start v = 1 + 0j
 *     lambda = conj(S * (1 / v));  v' = K lambda + L;  tol = max_i | |v'_i| - |v_i| |;  v = v'       (S = (P + jQ) / s_base, grid.py:151-199)
 * while iterations < max_iter and tol >= tolerance; |v| with the slack's 1.0 in front is env.node_voltage of that step, and the voltage
 * rewards add  loss_v = sum_i min(0, 0.05 - |1 - |v_i||)  over all n_bus entries (rl_agent/reward.py:117-119, 269-279).
 * K [n,n] and L [n] (n = n_bus - 1; complex128, re / im interleaved, HOST) are the network's -inv(Ydd) and K Yds (grid_tensor.py:110-118),
 * uploaded once.  The stopping rule is per env: an env that has converged keeps its v and its iteration count while others go on, and the loop
 * is bounded by max_iter whatever the data does (a NaN residual ends it, as numpy's comparison does).
 * Stated differences to the reference:
 *  - the product K lambda is summed over j = 0 .. n-1 in that order with fused multiply-adds; numpy's goes through BLAS in no defined order, so
 *    voltages agree to rounding (1e-9 relative is the bar the tests hold), not bit for bit; iteration counts agree wherever the residual is
 *    not within rounding of the tolerance;
 *  - the base profiles are the CALLER's arrays: the reference samples loads from a fitted generator (data/augmentor.pkl) that is not part of it;
 *  - the episode statistics (ev2g_get_stats' total_reward included) keep the step kernel's own reward; the composed reward is what
 *    ev2g_grid_run writes to `reward`, and its sum over the episode is ev2g_grid_get_stats' rew_sum;
 *  - ev2g_pool_refill does not re-draw a grid's profiles: they stay attached to the pool slots they were uploaded for.
 * Out of scope: the load-profile generator, the PandaPower solver, V2G_grid_full_reward (it needs a per-departure term of the step kernels),
 * saved_grid_energy (the reference never writes that array: 0) and fusing the grid or state kernels into a persistent step launch. */
typedef struct ev2g_grid ev2g_grid;
/* Needs loaded scenarios; freed with the handle if not before.  p_base / q_base: HOST arrays [M, T+1, n] in kW, block m for scenario m of the
 * resident pool (env e runs scenario (e + offset) mod M), row t read after step t (the reference also reads row T, after the last step) -- or
 * both NULL: a solver only (ev2g_grid_solve), ev2g_grid_run then fails.  EV2G_ERR_ARG: n_bus < 2 or > 1025, max_iter < 0, s_base <= 0, and --
 * with profiles -- a scenario batch whose transformer count is not n_bus - 1 (the reference builds one transformer per non-slack bus,
 * loaders.py:481-485).  The reference's settings are s_base 1000, tolerance 1e-6, max_iter 100 (grid_tensor.py:50,564-565). */
int ev2g_grid_create(ev2g_handle *h, int n_bus, const double *K, const double *L, double s_base, double tolerance, int max_iter,
                     const double *p_base, const double *q_base, ev2g_grid **out);
void ev2g_grid_destroy(ev2g_handle *h, ev2g_grid *g);
/* The bare batched solver, no engine state involved: p_kw / q_kw [n_rows, n] DEVICE in kW -> vm [n_rows, n_bus], v_complex [n_rows, n, 2],
 * iters [n_rows] int32, loss_v [n_rows] (DEVICE, each may be NULL).  Asynchronous on the handle's stream. */
int ev2g_grid_solve(ev2g_handle *h, ev2g_grid *g, const double *p_kw, const double *q_kw, int n_rows, double *vm, double *v_complex,
                    int32_t *iters, double *loss_v);
/* k_steps x ([agent ->] one-step launch of the step kernel the handle selected -> grid kernel) inside ONE episode, enqueued without host round
 * trips.  Arguments and error returns as ev2g_link_run (agent == NULL: actions [k,E,P] are read; EV2G_ERR_DONE for a segment past the episode
 * end).  After step t the grid kernel solves P_i = p_base[scenario, t, i] + transformer i's power, Q_i = q_base[scenario, t, i], writes |v| to
 * vm [k,E,n_bus] at base + k*v_stride (v_stride 0: one block; NULL: a block of the grid) and rewrites
 *     reward[e] = base_weight * reward[e] + voltage_weight * loss_v[e]          (base_weight == 0: voltage_weight * loss_v, nothing read)
 * V2G_grid_simple_reward is (0, 1000); Grid_V2G_profitmaxV2 is (1, 50000) on a handle whose reward is EV2G_REWARD_V2G_PROFITMAX_V2.
 * Timed like ev2g_step_n (ev2g_last_step_n_kernel_ms). */
int ev2g_grid_run(ev2g_handle *h, ev2g_grid *g, ev2g_heuristic *agent, int k_steps, double *actions, int64_t a_stride, double *obs,
                  int64_t o_stride, double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride,
                  double *vm, int64_t v_stride, double base_weight, double voltage_weight);
/* The episode's voltage statistics (get_statistics, utilities/utils.py:65-112), kept by the grid kernel of ev2g_grid_run / _run_observed /
 * _rollout: per env the sum of loss_v over the steps run (voltage_violation), the number of (step, non-slack bus) pairs with |v| < 0.95 or
 * |v| > 1.05 (voltage_violation_counter), the number of steps with at least one (voltage_violation_counter_per_step) and the sum of the
 * composed rewards written to `reward` (total_reward).  The step of counter 0 overwrites them: an episode restarts them itself, and a
 * segmented run reports what an unsplit one does.  HOST arrays [E], each may be NULL; synchronises the stream. */
int ev2g_grid_get_stats(ev2g_handle *h, ev2g_grid *g, double *vv_sum, int32_t *vv_count, int32_t *vv_steps, double *rew_sum);
/* ---- V2G_grid_state (rl_agent/state.py:216-278): the observation of the grid scenario, a property of a grid -- not an EV2G_STATE_* kind ----
 * Row of env e at step counter c (0 = after reset ... T = after the last step), Dg = 6 + 2n + 3P columns, n = n_bus - 1:
 *   0..2  weekday/7, sin(hour/24 2 pi), cos(hour/24 2 pi) of sim_date at c: time_features, a HOST table [M, T+1, 3] -- or [1, T+1, 3] with
 *         per_scenario == 0 -- copied as it is (the engine keeps no calendar);   3  charge_prices[0, c], signed, 0 at c == T;
 *   4  power_setpoints[c], 0 at c == T;   5  current_power_usage[c-1], 0 at c == 0;   6..6+n  p_base[scenario, c, :];   6+n..6+2n  q_base
 *   likewise (what node_active_power / node_reactive_power [1:, max(c-1, 0)] hold: PowerGrid.step returns the NEXT row's base, grid.py:131-141);
 *   then per port in reference port order (EV.current_capacity, time_of_departure - c + 1, the charger's transformer index) or three zeros.
 * Copies, integer differences and constants only: bit for bit the reference's row; float32 rows are the plain conversion of the float64 ones.
 * ev2g_grid_state_attach uploads the table and allocates the grid's own rows (EV2G_ERR_ARG for a solver-only grid); ev2g_grid_state_dim
 * returns Dg, or -1 without an attached state. */
int ev2g_grid_state_attach(ev2g_handle *h, ev2g_grid *g, const double *time_features, int per_scenario);
int ev2g_grid_state_dim(ev2g_handle *h, ev2g_grid *g);
/* The state of the handle's current step counter into obs [E,Dg] float64 and obs32 [E,Dg] float32 (DEVICE, each may be NULL) and into the
 * grid's own rows, which ev2g_grid_rollout starts from.  Asynchronous on the handle's stream. */
int ev2g_grid_observe(ev2g_handle *h, ev2g_grid *g, double *obs, float *obs32);
/* ev2g_grid_run, plus after each step's power flow the state of the NEXT counter into gobs [k,E,Dg] at base + k*go_stride and gobs32
 * likewise (DEVICE, stride 0: one block; gobs NULL: not written; gobs32 NULL: the grid's own float32 row, so that ev2g_grid_rollout can go on). */
int ev2g_grid_run_observed(ev2g_handle *h, ev2g_grid *g, ev2g_heuristic *agent, int k_steps, double *actions, int64_t a_stride, double *obs,
                           int64_t o_stride, double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride,
                           double *vm, int64_t v_stride, double base_weight, double voltage_weight, double *gobs, int64_t go_stride,
                           float *gobs32, int64_t go32_stride);
/* The policy loop on the grid scenario: k_steps x (ev2g_mlp_forward on the grid's float32 state row -> the float32 actions widened into a
 * float64 block -> one-step launch (no step-kernel observation) -> grid kernel -> state kernel into the float32 row), inside one episode,
 * enqueued without host round trips; reward / done / mask / vm as in ev2g_grid_run.  EV2G_ERR_ARG unless the actor maps Dg -> P;
 * EV2G_ERR_STATE unless the grid's row holds the state of the current counter: ev2g_grid_observe (or a previous ev2g_grid_rollout / an
 * ev2g_grid_run_observed with gobs32 NULL) wrote it and no reset or step outside these calls came after.  Timed like ev2g_step_n. */
int ev2g_grid_rollout(ev2g_handle *h, ev2g_grid *g, const ev2g_mlp *m, int k_steps, double *reward, int64_t r_stride, uint8_t *done,
                      int64_t d_stride, uint8_t *mask, int64_t m_stride, double *vm, int64_t v_stride, double base_weight, double voltage_weight);

/* ---- on-policy rollouts ON THE DEVICE: a Gaussian actor-critic and GAE (train_stable_baselines.py:24,62-130: PPO by default, A2C, TRPO) --------
 * SB3's default ActorCriticPolicy for a Box action space: a policy trunk d_in -> h1 -> h2 with a linear action head h2 -> d_out (the mean), a
 * separate value trunk d_in -> v1 -> v2 with a linear head v2 -> 1, one hidden activation for both trunks and a state-independent log_std[d_out].
 * Weights are HOST float32 arrays in torch.nn.Linear layout (W[out,in] row-major, b[out]), copied once.  Float32 operands on the exact-f32 matrix
 * instruction, float32 accumulation (csrc/ev2g_ac.h); no bf16 split.
 * LIMITS: d_in <= 192, every hidden width <= 256, d_out <= 64 -- the shipped V2G_profit_max_loads (162 -> 50) and PublicPST (63 -> 20) shapes fit;
 * anything else is EV2G_ERR_ARG at create, there is no generic fallback.
 * One launch per batch of observation rows computes both trunks and both heads and, when sampling,
 *     a = mean + exp(log_std) * eps,   log_prob = sum_p [ -(a - mean)^2 / (2 sigma^2) - log_std - log(2 pi) / 2 ]   on the UNCLIPPED a (as SB3 does),
 *     a_env = clip(a, lo, 1),  lo = -1 or 0: the reference's two action boxes, the meaning of ev2g_mlp's out_lo.
 * A row's results do not depend on which other rows are in the launch or where the row sits in it.  log_prob is summed in float64 and rounded once.
 * eps comes from a counter, not a stored stream: draw index j is Box-Muller on the uniforms 2 j and 2 j + 1 of ev2g_host_uniform's generator under
 * the object's seed, sqrt(-2 log(1 - u[2j])) cos(2 pi u[2j+1]) evaluated in float64 and rounded to float32; element (row e, port p) of the object's
 * n-th sampling launch over E rows draws index (n E + e) d_out + p.  n is a 64-bit counter of the object: every SAMPLING launch (ev2g_ac_act with
 * deterministic == 0, every step of such an ev2g_ac_collect) advances it by one, ev2g_ac_seed sets it.  ev2g_ac_host_normal is the host twin: the
 * same bits. */
#define EV2G_AC_TANH 0 /* SB3's default activation_fn */
#define EV2G_AC_RELU 1
typedef struct ev2g_acpolicy ev2g_acpolicy;
/* Needs a handle, not loaded scenarios; freed with the handle if not before.  pi_*: policy trunk, vf_*: value trunk, action_* / value_*: the two heads
 * (SB3's mlp_extractor.policy_net.{0,2}, mlp_extractor.value_net.{0,2}, action_net, value_net).  EV2G_ERR_ARG with a message naming the field: a
 * width outside the limits, an unknown activation, lo not -1 or 0, a log_std that is not finite. */
int ev2g_ac_create(ev2g_handle *h, int d_in, int h1, int h2, int v1, int v2, int d_out, int activation, const float *pi_W1, const float *pi_b1,
                   const float *pi_W2, const float *pi_b2, const float *vf_W1, const float *vf_b1, const float *vf_W2, const float *vf_b2,
                   const float *action_W, const float *action_b, const float *value_W, const float *value_b, const float *log_std, float lo,
                   uint64_t seed, ev2g_acpolicy **out);
void ev2g_ac_destroy(ev2g_handle *h, ev2g_acpolicy *ac);
/* the noise stream's seed and the launch counter n the next sampling launch uses */
int ev2g_ac_seed(ev2g_handle *h, ev2g_acpolicy *ac, uint64_t seed, uint64_t first_draw);
/* log_std [d_out] HOST (a learner changes it every update); the weights: same pointers as create, same shapes */
int ev2g_ac_set_log_std(ev2g_handle *h, ev2g_acpolicy *ac, const float *log_std);
int ev2g_ac_set_weights(ev2g_handle *h, ev2g_acpolicy *ac, const float *pi_W1, const float *pi_b1, const float *pi_W2, const float *pi_b2,
                        const float *vf_W1, const float *vf_b1, const float *vf_W2, const float *vf_b2, const float *action_W,
                        const float *action_b, const float *value_W, const float *value_b);
/* mean [n_rows, d_out] and value [n_rows] of obs32 [n_rows, d_in] (float32 DEVICE pointers, each output may be NULL): no sample is taken and no
 * counter advanced -- the bootstrap value of the row behind a segment, and the deterministic evaluation path.  Asynchronous on the handle's stream. */
int ev2g_ac_forward(ev2g_handle *h, ev2g_acpolicy *ac, const float *obs32, int n_rows, float *mean, float *value);
/* ONE sampling launch, no step: actions [n_rows, d_out] the unclipped sample (what SB3 stores), clipped [n_rows, d_out] what a step would read,
 * value / log_prob [n_rows] (float32 DEVICE, each may be NULL).  deterministic != 0: a = mean (EvalCallback(deterministic=True),
 * train_stable_baselines.py:82-87), nothing drawn, the counter stays. */
int ev2g_ac_act(ev2g_handle *h, ev2g_acpolicy *ac, const float *obs32, int n_rows, int deterministic, float *actions, float *clipped, float *value,
                float *log_prob);
/* On-policy ROLLOUT COLLECTION (the collect_rollouts() half of an SB3 PPO / A2C loop): k_steps x (the launch above on observation row i -> one-step
 * launch of the step kernel the handle selected, reading the object's clipped block and writing observation row i + 1) inside ONE episode, the rows
 * landing in the caller's DEVICE arrays.  d_in must be the handle's observation width and d_out its ports (EV2G_ERR_ARG); a segment that would run
 * past the episode end returns EV2G_ERR_DONE: statistics and reset in between are the caller's (ev2g_get_stats_reset_f32).  The two routes of
 * ev2g_collect's unfused loop: on the fast path the step takes the float32 rows per launch; elsewhere it works on the hand-over pair registered with
 * ev2g_set_step_extras (observation step stride 0; EV2G_ERR_ARG without it) and the rows are copied device-to-device around it.  Timed like
 * ev2g_step_n (ev2g_last_step_n_kernel_ms).  The chain is NOT captured into a graph and has NO fused-launch variant (ev2g_rollout's single launch
 * has no place for the sampling epilogue).  The entry takes no link, grid or action wrapper: the chain holds none of their stages (an
 * actor-critic is refused next to them inside one chain), and objects of those kinds that live on the handle are neither used nor touched. */
typedef struct ev2g_onpolicy_rows {
    float *obs;       /* [k_steps + 1, E, D]; row 0 read, rows 1.. written */
    float *actions;   /* [k_steps, E, P] the unclipped samples, written */
    float *values;    /* [k_steps, E] written */
    float *log_probs; /* [k_steps, E] written */
    double *reward;   /* [k_steps, E] written */
    uint8_t *done;    /* [k_steps, E] written */
    uint8_t *mask;    /* [k_steps, E, P] written */
} ev2g_onpolicy_rows;
int ev2g_ac_collect(ev2g_handle *h, ev2g_acpolicy *ac, int k_steps, int deterministic, const ev2g_onpolicy_rows *r);
/* dst [n_values] float32 HOST: the standard normals of draw indices first_index .. first_index + n_values - 1 under `seed` */
void ev2g_ac_host_normal(float *dst, int64_t n_values, uint64_t seed, uint64_t first_index);
/* SB3's RolloutBuffer.compute_returns_and_advantage in float32, one thread per env walking the k rows backwards, with g = (float)gamma and
 * c = (float)(gamma * lambda) (the float64 product rounded once):
 *     nnt = 1 - next_start;  delta = (r + (g * next_v) * nnt) - v;  adv = delta + (c * nnt) * last;  ret = adv + v;  r = (float)reward
 * reward [k, n_envs] float64, values [k, n_envs] float32, episode_starts [k, n_envs] uint8 (row t: step t is the first of an episode), last_values
 * [n_envs] float32 the value of the observation behind the last row, last_dones [n_envs] uint8 whether the last row ended an episode; advantages /
 * returns [k, n_envs] float32 written.  DEVICE pointers; ev2g_host_gae is the same function on HOST pointers (one source, the same bits).  n_envs is
 * passed explicitly -- the host twin has no handle to take it from, and the device entry works on any [k, n_envs] block, not only the handle's E. */
int ev2g_gae(ev2g_handle *h, const double *reward, const float *values, const uint8_t *episode_starts, const float *last_values,
             const uint8_t *last_dones, int k, int n_envs, double gamma, double lambda, float *advantages, float *returns);
int ev2g_host_gae(const double *reward, const float *values, const uint8_t *episode_starts, const float *last_values, const uint8_t *last_dones,
                  int k, int n_envs, double gamma, double lambda, float *advantages, float *returns);

/* ---- the learners of a Gaussian actor-critic (csrc/ev2g_ppo.h): PPO here, A2C below ------------
 * A learner object (struct ev2g_ppo, of either kind) belongs to one policy; a policy has at most one.
 * SB3's PPO.train() with default settings for ActorCriticPolicy on a Box action space, one minibatch per call, on the device: the forward with
 * every activation kept, the clipped-surrogate / value / entropy loss, backprop, clip_grad_norm_, torch.optim.Adam on float32 masters in SB3's
 * [out, in] layout, and the rewrite of the packed weight images the policy object's launches read.  float32 throughout, matrix products on the
 * exact-f32 MFMA.  No float atomics: the same call on the same state gives the same bits.
 *   lp_i = sum_p [ -(a - mu)^2 / (2 sigma^2) - log_std_p - log(2 pi) / 2 ] on the UNCLIPPED action;  r = exp(lp - old_lp)
 *   A^ = (A - mean(A)) / (std(A) + 1e-8) with the unbiased std, when normalize_advantage is set and B > 1, else A
 *   loss = -mean(min(A^ r, A^ clip(r, 1 - c, 1 + c))) + ent_coef * (-entropy) + vf_coef * mean((R - v)^2)
 *   statistics [6]: policy_loss, value_loss, entropy_loss, loss, approx_kl = mean((r - 1) - log r), clip_fraction = mean(|r - 1| > c)
 * Not reproduced (there is nothing to ask them with): clip_range_vf, target_kl, schedule objects (ev2g_ppo_set_rates between calls
 * drives one), action masks, orthogonal initialisation.
 * LIMITS: every network with d_in <= 192, d_out <= 64 and hidden widths <= 64 is accepted, wider ones as far as the gradient kernel's LDS plan
 * fits the CU's 160 KiB (ev2g_ppo_query tells); anything else is EV2G_ERR_ARG at create with a message naming the width. */
typedef struct ev2g_ppo ev2g_ppo;
typedef struct ev2g_ppo_config {
    double lr, beta1, beta2, adam_eps;   /* SB3's PPO: 3e-4, 0.9, 0.999, 1e-5.  lr >= 0, betas in [0, 1), adam_eps > 0 */
    double clip_range, vf_coef, ent_coef, max_grad_norm;   /* 0.2, 0.5, 0.0, 0.5.  clip_range > 0, coefficients >= 0, max_grad_norm > 0 */
    int32_t normalize_advantage;         /* 1 */
} ev2g_ppo_config;
typedef struct ev2g_ppo_info {
    int64_t lds_bytes, workspace_bytes;  /* the gradient kernel's dynamic LDS; the per-workgroup partial sums */
    int32_t grid_cap, n_params;          /* workgroups of the gradient kernel at most; elements of the thirteen arrays */
} ev2g_ppo_info;
/* Host-only (no GPU, no handle): the plan of a network's learner, or EV2G_ERR_ARG (ev2g_last_error(NULL) names the width). */
int ev2g_ppo_query(int d_in, int h1, int h2, int v1, int v2, int d_out, ev2g_ppo_info *info);
/* A learner bound to `ac` (created on `h`, one learner per policy: EV2G_ERR_STATE for a second), owned by the handle; the policy's current
 * weights and log_std become the masters, Adam's state starts at zero.  EV2G_ERR_ARG: a non-finite or out-of-range config value, a network the
 * plan refuses.  Destroying the policy destroys its learner.  While a learner is bound, ev2g_ac_set_weights / ev2g_ac_set_log_std also reset the
 * masters; Adam's m, v and step count are kept. */
int ev2g_ppo_create(ev2g_handle *h, ev2g_acpolicy *ac, const ev2g_ppo_config *cfg, ev2g_ppo **out);
void ev2g_ppo_destroy(ev2g_handle *h, ev2g_ppo *ppo);
int ev2g_ppo_set_rates(ev2g_handle *h, ev2g_ppo *ppo, double lr, double clip_range);
/* The gradient of one minibatch: rows idx[0 .. B) (int32, duplicates allowed, each inside the arrays) of obs [N, d_in], actions [N, d_out]
 * (unclipped), old_log_prob / advantages / returns [N]; all DEVICE, float32.  stats float32 [6] DEVICE, may be NULL.  The gradient stays in the
 * learner (unclipped).  Asynchronous on the handle's stream. */
int ev2g_ppo_grad(ev2g_handle *h, ev2g_ppo *ppo, const float *obs, const float *actions, const float *old_log_prob, const float *advantages,
                  const float *returns, const int32_t *idx, int B, float *stats);
/* clip_grad_norm_, Adam, repack: consumes the gradient of the last ev2g_ppo_grad (EV2G_ERR_STATE without one).  The policy's derived sigma is
 * NOT refreshed (ev2g_ppo_sync does that); the learner itself reads the master log_std. */
int ev2g_ppo_apply(ev2g_handle *h, ev2g_ppo *ppo);
/* ev2g_ppo_grad then ev2g_ppo_apply, no host round trip. */
int ev2g_ppo_minibatch(ev2g_handle *h, ev2g_ppo *ppo, const float *obs, const float *actions, const float *old_log_prob, const float *advantages,
                       const float *returns, const int32_t *idx, int B, float *stats);
/* The last gradient, unclipped, SB3's layout, into thirteen HOST arrays (the twelve of ev2g_ac_create's order, then log_std).  Synchronises. */
int ev2g_ppo_get_grads(ev2g_handle *h, ev2g_ppo *ppo, float *pi_W1, float *pi_b1, float *pi_W2, float *pi_b2, float *vf_W1, float *vf_b1,
                       float *vf_W2, float *vf_b2, float *action_W, float *action_b, float *value_W, float *value_b, float *log_std);
/* Synchronises, reads the master log_std back and re-derives the policy's sampling constants through ev2g_ac_set_log_std's path: afterwards the
 * policy samples exactly as a fresh one created from the same numbers.  Once per train(). */
int ev2g_ppo_sync(ev2g_handle *h, ev2g_ppo *ppo);
/* The policy's weights into twelve HOST arrays and log_std [d_out]: the masters when a learner is bound, else the packed images unpacked (and the
 * log_std last set).  Synchronises. */
int ev2g_ac_get_weights(ev2g_handle *h, ev2g_acpolicy *ac, float *pi_W1, float *pi_b1, float *pi_W2, float *pi_b2, float *vf_W1, float *vf_b1,
                        float *vf_W2, float *vf_b2, float *action_W, float *action_b, float *value_W, float *value_b, float *log_std);
/* Host twins (the device's element functions compiled for the host).  ev2g_host_adam: n elements of theta / m / v updated by gradient g at
 * step count t >= 1 (torch.optim.Adam, no amsgrad, no weight decay). */
int ev2g_host_adam(float *theta, float *m, float *v, const float *g, int64_t n, int64_t t, double lr, double beta1, double beta2, double eps);
/* ev2g_host_ppo_head: one minibatch's head gradients d loss / d mean [B, P], d loss / d value [B], d loss / d log_std [P] (entropy term included)
 * and the six statistics, from given mean [B, P], value [B], actions [B, P], log_std [P], old_log_prob / advantages / returns [B]. */
int ev2g_host_ppo_head(const float *mean, const float *value, const float *actions, const float *log_std, const float *old_log_prob,
                       const float *advantages, const float *returns, int B, int P, const ev2g_ppo_config *cfg, float *d_mean, float *d_value,
                       float *d_log_std, float *stats);

/* ---- the A2C learner: SB3's A2C.train() with default settings, one update per call over the rows it is given ----
 * The same learner object, gradient kernel (with a ratio-free head, a compile-time choice), reduction and limits as PPO's; the optimiser is
 * torch.optim.RMSprop, which is what SB3's A2C builds by default.
 *   lp_i as above;  A^ = (A - mean(A)) / (std(A) + 1e-8), unbiased std, if normalize_advantage (default off), else A
 *   loss = -mean(A^ lp) + ent_coef * (-entropy) + vf_coef * mean((R - v)^2);   g <- g * min(1, max_grad_norm / (|g| + 1e-6))
 *   RMSprop(lr, alpha, eps, no weight decay, no momentum, not centered): sq <- alpha sq + (1 - alpha) g g;  theta <- theta - lr g / (sqrt(sq) + eps)
 *   statistics [6] in ev2g_ppo_grad's order; approx_kl and clip_fraction are exactly 0.
 * use_rms_prop = 0 selects torch.optim.Adam(betas 0.9 / 0.999, eps 1e-5), what SB3's policy builds when RMSprop is switched off.
 * Not reproduced: RMSpropTFLike, schedule objects (ev2g_a2c_set_rate between calls drives one), action masks.  (TRPO is the third kind, below.)
 * ev2g_ppo_destroy, ev2g_ppo_get_grads, ev2g_ppo_sync, ev2g_ppo_query and ev2g_ac_get_weights serve both kinds, and ev2g_ac_set_weights /
 * ev2g_ac_set_log_std reset the masters of both (the optimiser's state is kept).  ev2g_ppo_grad / _apply / _minibatch / _set_rates on an A2C
 * learner, and the ev2g_a2c_* entries on a PPO learner, are EV2G_ERR_STATE. */
typedef struct ev2g_a2c_config {
    double lr, alpha, rms_eps;                 /* SB3's A2C: 7e-4, 0.99, 1e-5.  lr >= 0, alpha in [0, 1), rms_eps > 0 */
    double vf_coef, ent_coef, max_grad_norm;   /* 0.5, 0.0, 0.5.  coefficients >= 0, max_grad_norm > 0 */
    int32_t normalize_advantage;               /* 0 */
    int32_t use_rms_prop;                      /* 1; 0: Adam(0.9, 0.999, eps 1e-5) */
} ev2g_a2c_config;
/* As ev2g_ppo_create: one learner per policy of either kind (EV2G_ERR_STATE for a second), the same accepted networks, EV2G_ERR_ARG naming the
 * field for a non-finite or out-of-range config value.  The optimiser's state starts at zero. */
int ev2g_a2c_create(ev2g_handle *h, ev2g_acpolicy *ac, const ev2g_a2c_config *cfg, ev2g_ppo **out);
int ev2g_a2c_set_rate(ev2g_handle *h, ev2g_ppo *learner, double lr);
/* The gradient of one update over rows idx[0 .. B) of the DEVICE float32 arrays (as ev2g_ppo_grad, without old_log_prob): duplicates allowed,
 * B >= 1; normalize_advantage with B == 1 is EV2G_ERR_ARG (SB3 would produce NaN).  stats float32 [6] DEVICE, may be NULL. */
int ev2g_a2c_grad(ev2g_handle *h, ev2g_ppo *learner, const float *obs, const float *actions, const float *advantages, const float *returns,
                  const int32_t *idx, int B, float *stats);
/* clip_grad_norm_, the optimiser's step, repack: consumes the gradient of the last ev2g_a2c_grad (EV2G_ERR_STATE without one). */
int ev2g_a2c_apply(ev2g_handle *h, ev2g_ppo *learner);
/* ev2g_a2c_grad then ev2g_a2c_apply, no host round trip. */
int ev2g_a2c_update(ev2g_handle *h, ev2g_ppo *learner, const float *obs, const float *actions, const float *advantages, const float *returns,
                    const int32_t *idx, int B, float *stats);
/* Host twins.  ev2g_host_rmsprop: n elements of theta / sq updated by gradient g (torch.optim.RMSprop as above).  ev2g_host_a2c_head: as
 * ev2g_host_ppo_head with A2C's head. */
int ev2g_host_rmsprop(float *theta, float *sq, const float *g, int64_t n, double lr, double alpha, double eps);
int ev2g_host_a2c_head(const float *mean, const float *value, const float *actions, const float *log_std, const float *advantages,
                       const float *returns, int B, int P, const ev2g_a2c_config *cfg, float *d_mean, float *d_value, float *d_log_std, float *stats);

/* ---- the TRPO learner (csrc/ev2g_trpo.h): sb3_contrib's TRPO.train() with default settings ----
 * A third kind of the same learner object.  The POLICY STEP, over the rows it is given, entirely on the handle's stream (no host round trip):
 *   A^ as above (normalised when normalize_advantage is set and B > 1);  J(theta) = mean(A^ exp(lp - old_lp));  g = grad J over the ACTOR's
 *   parameters, flat in sb3_contrib's order: log_std | pi_W1 | pi_b1 | pi_W2 | pi_b2 | action_W | action_b
 *   KL(theta) = mean_i sum_p [ ls0_p - ls_p + (e^{2 ls_p} + (mu_ip - mu0_ip)^2) / (2 e^{2 ls0_p}) - 1/2 ]  (new || old; mu0, ls0 at theta0)
 *   H v = grad(grad KL . v) + cg_damping v, computed as the Fisher product J_mu^T diag(e^{-2 ls0}) J_mu v / B + 2 v_log_std + cg_damping v
 *   (exact at theta0: one forward-mode tangent pass, then the reverse pass)
 *   conjugate gradient on H x = g: x = 0, r = p = g, rho = r . r; nothing if rho < 1e-10; at most cg_max_steps times alpha = rho / (p . Hp),
 *   x += alpha p, and unless it was the last: r -= alpha Hp, rho' = r . r, stop if rho' < 1e-10, p = r + (rho' / rho) p
 *   beta = sqrt(2 target_kl / (x . Hx));  line search: theta = theta0 + c beta x for c = 1, s, s^2, ... (at most line_search_max_iter tries),
 *   accepted when KL < target_kl and J > J(theta0); theta0 is put back bit for bit when no try is.
 * DEVIATION: a non-finite or non-positive x . Hx (x = 0 from a vanishing gradient included) fails the step and leaves theta0; sb3_contrib
 * would write NaN parameters.
 * The CRITIC: value_loss = mean((R - v)^2) over a minibatch, torch.optim.Adam(lr, 0.9, 0.999, eps 1e-5) on the six value arrays alone, no
 * gradient clipping; the actor's arrays, their images and their optimiser slots are not touched.
 * Not reproduced: use_sde, shared trunks, schedule objects (ev2g_trpo_set_rate between calls drives one), action masks.
 * ev2g_ppo_destroy, ev2g_ppo_sync, ev2g_ppo_get_grads and ev2g_ac_get_weights serve this kind too; the other ev2g_ppo_* and the ev2g_a2c_*
 * entries on a TRPO learner, and the ev2g_trpo_* entries on another kind, are EV2G_ERR_STATE. */
typedef struct ev2g_trpo_config {
    double lr;                                 /* 1e-3: the value function's Adam.  lr >= 0 */
    double target_kl, cg_damping;              /* 0.01, 0.1.  target_kl > 0, cg_damping >= 0 */
    double line_search_shrinking_factor;       /* 0.8, in (0, 1) */
    int32_t cg_max_steps, line_search_max_iter;   /* 15, 10.  both >= 1 */
    int32_t normalize_advantage;               /* 1 */
} ev2g_trpo_config;
typedef struct ev2g_trpo_info {
    int64_t lds_bytes, workspace_bytes;        /* the kernels' dynamic LDS (never more than ev2g_ppo_query's); slabs + the solve's vectors */
    int32_t grid_cap, n_params, n_actor;       /* as ev2g_ppo_info; elements of a flat actor vector */
} ev2g_trpo_info;
typedef struct ev2g_trpo_report {
    int32_t cg_iterations, line_search_tries, accepted, failed;   /* failed: no try was made (x . Hx not positive) */
    double objective_before, objective_after;  /* J(theta0); J of the last try evaluated (0 when none was) */
    double kl, beta, c, xHx;                   /* KL of the last try evaluated; the full step; the last coefficient; x . Hx, damping included */
} ev2g_trpo_report;
/* Host-only: the plan of a network's TRPO learner.  Accepts exactly what ev2g_ppo_query accepts. */
int ev2g_trpo_query(int d_in, int h1, int h2, int v1, int v2, int d_out, ev2g_trpo_info *info);
/* As ev2g_ppo_create: one learner per policy of any kind (EV2G_ERR_STATE for a second), EV2G_ERR_ARG naming the field for an out-of-range value. */
int ev2g_trpo_create(ev2g_handle *h, ev2g_acpolicy *ac, const ev2g_trpo_config *cfg, ev2g_ppo **out);
int ev2g_trpo_set_rate(ev2g_handle *h, ev2g_ppo *learner, double lr);
/* g, J(theta0) and mu0 over rows idx[0 .. B) of the DEVICE float32 arrays (as ev2g_ppo_grad, without returns).  g goes into the actor's seven
 * arrays of the gradient ev2g_ppo_get_grads reads; the six value arrays of it are untouched.  objective: float64 [1] DEVICE, may be NULL. */
int ev2g_trpo_grad(ev2g_handle *h, ev2g_ppo *learner, const float *obs, const float *actions, const float *old_log_prob, const float *advantages,
                   const int32_t *idx, int B, double *objective);
/* One product: v [n_actor] -> H v [n_actor], both DEVICE float32, flat in the actor's order, at the current parameters, cg_damping included. */
int ev2g_trpo_fvp(ev2g_handle *h, ev2g_ppo *learner, const float *obs, const int32_t *idx, int B, const float *v, float *Hv);
/* The whole policy step.  Asynchronous: ev2g_trpo_get_report (or ev2g_ppo_sync) waits for it. */
int ev2g_trpo_policy_step(ev2g_handle *h, ev2g_ppo *learner, const float *obs, const float *actions, const float *old_log_prob,
                          const float *advantages, const int32_t *idx, int B);
/* One critic minibatch: the value gradient over rows idx[0 .. B), then Adam.  value_loss: float32 [1] DEVICE, may be NULL. */
int ev2g_trpo_critic_minibatch(ev2g_handle *h, ev2g_ppo *learner, const float *obs, const float *returns, const int32_t *idx, int B, float *value_loss);
/* What the last ev2g_trpo_policy_step did (EV2G_ERR_STATE before the first).  Synchronises. */
int ev2g_trpo_get_report(ev2g_handle *h, ev2g_ppo *learner, ev2g_trpo_report *report);
/* The last step's x and g, flat in the actor's order, into HOST float64 arrays [n_actor] (either may be NULL).  EV2G_ERR_STATE before the first
 * step.  Synchronises. */
int ev2g_trpo_get_direction(ev2g_handle *h, ev2g_ppo *learner, double *x, double *g);
/* Host twins.  ev2g_host_trpo_cg_step: one iteration of the solve's vector algebra from a given Hp, x / r / p [n] float64 updated in place,
 * *rho in and out; returns through *done whether the solve has ended (the last iteration, or rho' < 1e-10).  ev2g_host_trpo_rows: the row terms
 * of J and KL, j / kl [B] float64, from mean / mean0 / actions [B, P], log_std / log_std0 [P], old_log_prob / advantages [B]. */
int ev2g_host_trpo_cg_step(double *x, double *r, double *p, const double *Hp, int64_t n, double *rho, int last, int32_t *done);
int ev2g_host_trpo_rows(const float *mean, const float *mean0, const float *actions, const float *log_std, const float *log_std0,
                        const float *old_log_prob, const float *advantages, int B, int P, int normalize_advantage, double *j, double *kl);

/* ---- the off-policy learner of the device replay ring: SB3's TD3.train() for TD3Policy, with DDPG as a preset (csrc/ev2g_td3.h) ----
 * One gradient step per call on a batch (s, a, r, s', done) of B rows, the update counter n incremented first:
 *   eps = clamp(target_policy_noise * N(0, 1), -target_noise_clip, +target_noise_clip);  a' = clamp(actor_target(s') + eps, -1, 1)
 *   y = r + ((1 - done) * gamma) * min_j critic_target_j(s', a');  critic_loss = sum_j mean((critic_j(s, a~) - y)^2) -> Adam over all critics
 *   n % policy_delay == 0: actor_loss = -mean(critic_0(s, actor(s))), critic_0 AFTER its step -> Adam on the actor, then
 *                          target <- (1 - tau) * target + tau * param for the critics and the actor (SB3's polyak_update)
 * Networks: actor d_in -> h1 -> h2 -> d_out (ReLU, tanh), each critic (d_in + d_out) -> h1 -> h2 -> 1 (ReLU), the hidden widths of the bound policy.
 * torch.optim.Adam with TD3Policy's eps 1e-8, no gradient clipping.  float32 throughout, every sum in one fixed order, no float atomics: the same
 * call on the same state gives the same bits.  Everything is enqueued on the handle's stream; no host round trip happens inside an update.
 * ACTIONS: `actions` holds what the replay ring stores, the env's action in [lo, 1] (lo: the bound policy's out_lo).  The critics take SB3's scaled
 * action in [-1, 1]: the learner reads a~ = 2 a - 1 when lo = 0 and a itself when lo = -1.  `done` is used as stored (the reference registers
 * no time limit and returns truncated = False: SB3 treats its episode ends as terminal).  reward is float32, as SB3's buffer stores it.
 * NOISE: element (row b, port p) of a noisy update draws standard normal index next_draw + b * d_out + p of ev2g_ac_host_normal's generator under
 * the learner's seed; next_draw then advances by B * d_out.  target_policy_noise = 0 draws nothing and advances nothing.
 * LIMITS (a message per field otherwise): d_in <= 192, d_out <= 64, hidden widths 1 .. 400, 1 <= B <= EV2G_TD3_MAX_BATCH, n_critics 1 or 2.
 * THE BOUND POLICY: ev2g_td3_create takes the ev2g_mlp that ev2g_collect / ev2g_rollout / ev2g_mlp_forward run and the actor's six float32
 * arrays as masters; it rewrites the policy's packed images from them at creation and after every actor step, in the precision the policy was
 * created with (every packing of csrc/ev2g_policy_host.h, padding untouched), so the collector reads the new actor without the weights leaving
 * the device.  A policy has at most one learner (EV2G_ERR_STATE for a second); the learner is owned by the handle and ends with it, with
 * ev2g_td3_destroy, or with ev2g_mlp_destroy of its policy.  Rollout graphs captured for the policy stay valid (the images keep their addresses).
 * Not reproduced: action_noise, learning_starts, schedule objects (ev2g_td3_set_rate between calls drives one).  SAC and TQC are not this
 * learner's: each has its own object with a stochastic actor, ev2g_sac_* and ev2g_tqc_* below. */
#define EV2G_TD3_MAX_BATCH 1024
typedef struct ev2g_td3 ev2g_td3;
typedef struct ev2g_td3_config {
    double lr, beta1, beta2, adam_eps;                     /* 1e-3, 0.9, 0.999, 1e-8.  lr >= 0, betas in [0, 1), adam_eps > 0 */
    double tau, gamma;                                     /* 0.005, 0.99.  both in [0, 1] */
    double target_policy_noise, target_noise_clip;         /* TD3: 0.2, 0.5; DDPG: 0, 0.5.  finite and >= 0 */
    int32_t n_critics, policy_delay;                       /* TD3: 2, 2; DDPG: 1, 1.  n_critics 1 or 2, policy_delay >= 1 */
} ev2g_td3_config;
/* SB3's defaults of TD3 (ddpg == 0) or of DDPG (ddpg != 0: one critic, no delay, no target noise) */
int ev2g_td3_default_config(int ddpg, ev2g_td3_config *cfg);
/* actor: six HOST float32 arrays W1 [h1, d_in], b1, W2 [h2, h1], b2, W3 [d_out, h2], b3 (d_in, h1, h2, d_out must be the policy's widths: EV2G_ERR_ARG); critics:
 * 6 * n_critics HOST arrays, critic j's W1 [h1, d_in + d_out], b1, W2 [h2, h1], b2, W3 [1, h2], b3 [1] at [6 j, 6 j + 6).  The targets start as
 * copies, Adam's state at zero.  Synchronises. */
int ev2g_td3_create(ev2g_handle *h, ev2g_mlp *policy, const ev2g_td3_config *cfg, int d_in, int h1, int h2, int d_out, const float *const *actor,
                    const float *const *critics, uint64_t seed, ev2g_td3 **out);
void ev2g_td3_destroy(ev2g_handle *h, ev2g_td3 *t);
/* One gradient step: obs / next_obs [B, d_in], actions [B, d_out], reward [B] float32, done [B] uint8, contiguous DEVICE arrays; losses float32
 * [2] DEVICE (critic_loss; actor_loss, written only by an update that steps the actor), may be NULL. */
int ev2g_td3_update(ev2g_handle *h, ev2g_td3 *t, const float *obs, const float *actions, const float *reward, const float *next_obs,
                    const uint8_t *done, int B, float *losses);
/* The two gradient stages without the apply.  ev2g_td3_critic_grad leaves the critics' gradient and y in the learner and draws the noise;
 * ev2g_td3_actor_grad leaves the actor's gradient (through critic_0 as it is now).  ev2g_td3_apply consumes the pending one (EV2G_ERR_STATE
 * without one): for a critic gradient Adam on the critics and n += 1; for an actor gradient Adam on the actor, the Polyak step and the
 * rewrite of the bound policy's images.  ev2g_td3_update is critic_grad, apply and -- when n % policy_delay == 0 -- actor_grad, apply.
 * Both halves may be pending at once (ev2g_td3_actor_grad after ev2g_td3_critic_grad without an apply in between: the actor's gradient through
 * critic_0 BEFORE its step); ev2g_td3_apply then consumes both, the critics' first, and drops neither.  Computing a half again replaces it. */
int ev2g_td3_critic_grad(ev2g_handle *h, ev2g_td3 *t, const float *obs, const float *actions, const float *reward, const float *next_obs,
                         const uint8_t *done, int B, float *losses);
int ev2g_td3_actor_grad(ev2g_handle *h, ev2g_td3 *t, const float *obs, int B, float *losses);
int ev2g_td3_apply(ev2g_handle *h, ev2g_td3 *t);
/* out: 6 + 6 * n_critics HOST arrays in SB3's parameter order (the actor's six, then each critic's six), each may be NULL.  get_grads: the
 * last gradient of each half.  get_weights: the masters (target == 0) or the target networks (target != 0).  ev2g_td3_get_y: y [B] of the last
 * critic gradient (B: its batch size).  All synchronise.  ev2g_td3_get_y and ev2g_td3_counters below are read-only additions for tests and
 * for TD3Learner.train()'s update count: nothing else depends on them. */
int ev2g_td3_get_grads(ev2g_handle *h, ev2g_td3 *t, float *const *out);
int ev2g_td3_get_weights(ev2g_handle *h, ev2g_td3 *t, int target, float *const *out);
int ev2g_td3_get_y(ev2g_handle *h, ev2g_td3 *t, float *y, int B);
int ev2g_td3_set_rate(ev2g_handle *h, ev2g_td3 *t, double lr);
/* the noise stream's seed and the draw index the next noisy update starts at */
int ev2g_td3_seed(ev2g_handle *h, ev2g_td3 *t, uint64_t seed, uint64_t first_draw);
/* updates applied to the critics (n), actor steps (each one a refresh of the bound policy), the next draw index; each may be NULL */
int ev2g_td3_counters(ev2g_handle *h, ev2g_td3 *t, int64_t *updates, int64_t *actor_steps, uint64_t *next_draw);
/* ---- the uniform sampler of a device replay ring of episode blocks ----
 * A block holds one episode of E envs: obs [T + 1, E, D] float32 (row t + 1 is row t's next observation, row T the terminal one), actions
 * [T, E, P] float32, reward [T, E] float64, done [T, E] uint8.  The ring lists its COMPLETE blocks only (HOST arrays of n_blocks DEVICE pointers
 * each, n_blocks <= 32).  Row i of draw `counter` reads the uniforms 3 j, 3 j + 1, 3 j + 2 of ev2g_host_uniform's generator under `seed`, j =
 * counter * EV2G_TD3_MAX_BATCH + i, and picks (entry of the list, t, e) as min(floor(u * n), n - 1) for n = n_blocks, T, E: a pure function of
 * (seed, counter, row, bounds), which ev2g_host_replay_indices repeats on the host.  The row's s, a, (float) r, s' = obs[t + 1, e] and done go to
 * the contiguous DEVICE batch arrays; index int32 [B, 3] DEVICE (may be NULL) receives the picks.  1 <= B <= EV2G_TD3_MAX_BATCH.  The caller
 * advances `counter` by one per draw.  Asynchronous on the handle's stream. */
typedef struct ev2g_replay_ring {
    int32_t n_blocks, T, E, D, P;
    const float *const *obs;
    const float *const *actions;
    const double *const *reward;
    const uint8_t *const *done;
} ev2g_replay_ring;
int ev2g_replay_sample(ev2g_handle *h, const ev2g_replay_ring *ring, int B, uint64_t seed, uint64_t counter, float *obs, float *actions,
                       float *reward, float *next_obs, uint8_t *done, int32_t *index);
int ev2g_host_replay_indices(int32_t *index, int B, int n_blocks, int T, int E, uint64_t seed, uint64_t counter);
/* Host twins of the learner's element functions.  ev2g_host_td3_target: a_next [B, P] = clamp(a_target + clamp(sigma N, -clip, clip), -1, 1) with
 * the draws first_draw + b P + p under `seed` (tq == NULL: only that), and -- given the target critics' values tq [n_critics, B] the caller
 * computed on (s', a_next) -- y [B].  ev2g_host_polyak: n elements of target moved towards param. */
int ev2g_host_td3_target(const float *a_target, const float *tq, const float *reward, const uint8_t *done, int B, int P, int n_critics, double sigma,
                         double clip, double gamma, uint64_t seed, uint64_t first_draw, float *a_next, float *y);
int ev2g_host_polyak(float *target, const float *param, int64_t n, double tau);

/* ---- SAC on the device: SB3's SAC.train() for SACPolicy (MlpPolicy, Box actions, use_sde off), and its stochastic collection actor
 * (csrc/ev2g_sac.h) ----
 *   actor: h = ReLU(W2 ReLU(W1 s + b1) + b2), mu = Wmu h + bmu, log_std = clamp(Wls h + bls, -20, 2), a = tanh(mu + exp(log_std) eps),
 *          log pi = sum_p [-eps^2 / 2 - log_std - log(2 pi) / 2] - sum_p log(1 - a^2 + 1e-6)
 *   critics: n_critics (1 or 2) of (s, a) -> h1 -> h2 -> 1 with ReLU, and their targets; no actor target.
 * One update on the contiguous DEVICE batch (s, a~, r, s', done) of B rows, alpha = exp(log_ent_coef) as it stands before the update, d the
 * learner's draw base (ev2g_sac_seed):
 *   a_pi, log pi on s with the draws d + b P + p;  a', log pi' on s' with the draws d + B P + b P + p;
 *   y = r + ((1 - done) gamma) (min_j target_j(s', a') - alpha log pi');  critic_loss = 0.5 sum_j mean((Q_j(s, a~) - y)^2) -> Adam on the critics;
 *   actor_loss = mean(alpha log pi - min_j Q_j(s, a_pi)) with the critics after their step, through each row's argmin critic -> Adam on the actor;
 *   ent_coef_loss = -mean(log_ent_coef (log pi + target_entropy)) -> Adam on log_ent_coef (ent_coef_auto only);
 *   every target_update_interval-th update target <- (1 - tau) target + tau param for the critics; d += 2 B P;
 *   the collection actor's packed weights are rewritten from the float32 masters.
 * `actions` holds what the replay ring stores, the env's action in [lo, 1]; the critics read SB3's scaled action (2 a - 1 for lo = 0).
 * float32 layer products, the heads in float64 from the stored float32 mu, raw log_std and eps with every output rounded once, every sum in one
 * fixed order, no float atomics: the same call on the same state gives the same bits.
 * LIMITS (a message per field otherwise): d_in <= 192, hidden widths 1 .. 256, d_out <= 64, 1 <= B <= EV2G_TD3_MAX_BATCH, n_critics 1 or 2.
 * actor: the 8 host arrays actor.latent_pi.{0,2}.{weight,bias}, actor.mu.{weight,bias}, actor.log_std.{weight,bias}; critics: 6 per critic; all
 * float32 in SB3's [out, in] layout.  The object belongs to the handle: freed by ev2g_sac_destroy or with ev2g_destroy.
 * Not reproduced: use_sde, action_noise, learning_starts, schedule objects (ev2g_sac_set_rate between calls drives one).  TQC's quantile
 * critics are not this object's: ev2g_tqc_* below. */
typedef struct ev2g_sac ev2g_sac;
typedef struct ev2g_sac_config {
    double lr, beta1, beta2, adam_eps, tau, gamma;         /* 3e-4 (all three optimisers), 0.9, 0.999, 1e-8, 0.005, 0.99 */
    double ent_coef;                                       /* the coefficient log_ent_coef starts from ("auto": 1.0, "auto_0.1": 0.1), or the fixed one.  > 0 */
    double target_entropy;                                 /* read when target_entropy_auto == 0 */
    int32_t n_critics, target_update_interval;             /* 2, 1 */
    int32_t ent_coef_auto, target_entropy_auto;            /* 1: log_ent_coef is trained; 1: target_entropy = -d_out */
} ev2g_sac_config;
int ev2g_sac_default_config(ev2g_sac_config *cfg);
int ev2g_sac_create(ev2g_handle *h, const ev2g_sac_config *cfg, int d_in, int h1, int h2, int d_out, float lo, const float *const *actor,
                    const float *const *critics, uint64_t seed, ev2g_sac **out);
void ev2g_sac_destroy(ev2g_handle *h, ev2g_sac *s);
/* losses (DEVICE float32 [4], may be NULL): critic_loss, actor_loss, ent_coef_loss (0 for a fixed coefficient), ent_coef.  Asynchronous. */
int ev2g_sac_update(ev2g_handle *h, ev2g_sac *s, const float *obs, const float *actions, const float *reward, const float *next_obs,
                    const uint8_t *done, int B, float *losses);
/* The two gradient stages without the apply.  ev2g_sac_critic_grad draws eps' (base d + B P) and leaves y, log pi' and the critics' gradient;
 * ev2g_sac_actor_grad draws eps (base d) and leaves log pi, the actor's gradient through the critics as they are now and the gradient of
 * log_ent_coef.  ev2g_sac_apply consumes what is pending (EV2G_ERR_STATE when nothing is), the critics' half first; applying an actor half
 * steps log_ent_coef, advances d by 2 B P, counts one update (the Polyak step on every target_update_interval-th) and rewrites the packed
 * weights.  ev2g_sac_update is critic_grad, apply, actor_grad, apply. */
int ev2g_sac_critic_grad(ev2g_handle *h, ev2g_sac *s, const float *obs, const float *actions, const float *reward, const float *next_obs,
                         const uint8_t *done, int B, float *losses);
int ev2g_sac_actor_grad(ev2g_handle *h, ev2g_sac *s, const float *obs, int B, float *losses);
int ev2g_sac_apply(ev2g_handle *h, ev2g_sac *s);
/* The collection actor on n_rows DEVICE observation rows [n_rows, d_in]: actions [n_rows, d_out] in the env's box [lo, 1]; mu, log_std (raw,
 * before the clamp) [n_rows, d_out] and log_pi [n_rows] may be NULL.  deterministic != 0: a = tanh(mu), nothing is drawn and the collection
 * counter does not move; else element (e, p) of the object's n-th sampling launch takes draw (n n_rows + e) d_out + p of the collection stream
 * (ev2g_sac_act_seed), which is not the learner's.  A row's outputs do not depend on the rows it is launched with. */
int ev2g_sac_act(ev2g_handle *h, ev2g_sac *s, const float *obs32, int n_rows, int deterministic, float *actions, float *mu, float *log_std,
                 float *log_pi);
/* ev2g_collect's unfused loop with ev2g_sac_act in the actor's place (same arrays, same refusals, the registered hand-over route included) */
int ev2g_sac_collect(ev2g_handle *h, ev2g_sac *s, int k_steps, int deterministic, const ev2g_transitions *tr);
/* Read-backs into HOST arrays; all synchronise.  `out`: 8 + 6 n_critics float32 arrays in SB3's parameter order (NULL entries skipped).
 * get_grads: the last gradient of each half, g_log_ent_coef (may be NULL) that of log_ent_coef.  get_weights: the masters (target == 0) or the
 * target critics (target != 0: the actor's 8 entries are not written).  get_y / get_log_pi: y and log pi' [B] of the last critic gradient / log pi
 * [B] of the last actor gradient.  get_ent_coef: out3 = {log_ent_coef, Adam's m, Adam's v}. */
int ev2g_sac_get_grads(ev2g_handle *h, ev2g_sac *s, float *const *out, float *g_log_ent_coef);
int ev2g_sac_get_weights(ev2g_handle *h, ev2g_sac *s, int target, float *const *out);
int ev2g_sac_get_y(ev2g_handle *h, ev2g_sac *s, float *y, float *log_pi_next, int B);
int ev2g_sac_get_log_pi(ev2g_handle *h, ev2g_sac *s, float *log_pi, int B);
int ev2g_sac_get_ent_coef(ev2g_handle *h, ev2g_sac *s, float *out3);
int ev2g_sac_set_rate(ev2g_handle *h, ev2g_sac *s, double lr);
/* the learner's noise stream: its seed and the base d of the next update; and the collection stream: its seed and the launch counter n */
int ev2g_sac_seed(ev2g_handle *h, ev2g_sac *s, uint64_t seed, uint64_t first_draw);
int ev2g_sac_act_seed(ev2g_handle *h, ev2g_sac *s, uint64_t seed, uint64_t first_launch);
/* updates applied, Polyak steps among them, the learner's next draw base, the collection stream's launch counter (each may be NULL) */
int ev2g_sac_counters(ev2g_handle *h, ev2g_sac *s, int64_t *updates, int64_t *target_updates, uint64_t *next_draw, uint64_t *act_launches);
/* Host twins of the head's element functions (HOST arrays).  ev2g_host_sac_head: a [B, P] (tanh), a_env [B, P] in [lo, 1] (may be NULL) and
 * log_pi [B] from mu, raw log_std and the standard normals eps [B, P].  ev2g_host_sac_head_back: d_mu, d_log_std [B, P] from g = dQ_min / da.
 * ev2g_host_sac_y: y [B] from the target critics' values tq [n_critics, B] and log pi' [B]. */
int ev2g_host_sac_head(const float *mu, const float *log_std, const float *eps, int B, int P, float lo, float *a, float *a_env, float *log_pi);
int ev2g_host_sac_head_back(const float *mu, const float *log_std, const float *eps, const float *g, int B, int P, float log_ent_coef, float *d_mu,
                            float *d_log_std);
int ev2g_host_sac_y(const float *tq, const float *log_pi_next, const float *reward, const uint8_t *done, int B, int n_critics, double gamma,
                    float log_ent_coef, float *y);

/* ---- TQC on the device: sb3_contrib's TQC.train() (Truncated Quantile Critics; MlpPolicy, Box actions, use_sde off) and its stochastic
 * collection actor (csrc/ev2g_tqc.h over csrc/ev2g_sac.h) ----
 *   actor: SAC's squashed Gaussian, bit for bit (the section above): the same head, draws, collection kernel and packed images.
 *   critics: n_critics (1 .. 5) of (s, a) -> h1 -> h2 -> n_quantiles (1 .. 64) with ReLU, no output activation, and their targets.
 *   nq = n_quantiles, nc = n_critics, d = top_quantiles_to_drop_per_net, M = nc nq <= 128 pooled atoms, K = M - d nc >= 1 kept target atoms,
 *   tau_i = (i + 0.5) / nq.
 * One update on the contiguous DEVICE batch (s, a~, r, s', done) of B rows, alpha = exp(log_ent_coef) as it stands before the update, the
 * draws as in SAC (a_pi: d0 + b P + p; a': d0 + B P + b P + p; d0 += 2 B P):
 *   per row the M atoms critic_target_j(s', a')[i] pooled j-major, sorted ascending under the key (value, pool index) -- equal values, +0 and
 *   -0 among them, keep their pool order -- and the first K kept:  z_k = r + ((1 - done) gamma) (sorted_k - alpha log pi');
 *   delta = z_k - critic_j(s, a~)[i];  critic_loss = mean over (b, j, i, k) of |tau_i - 1[delta < 0]| huber(delta), huber = |delta| - 0.5 where
 *   |delta| > 1 else 0.5 delta^2 (one plain mean, sum_over_quantiles = False) -> Adam on all critics;
 *   actor_loss = mean_b(alpha log pi_b - mean_{j,i} critic_j(s, a_pi)[i]) with the critics after their step, through every critic -> Adam on the actor;
 *   ent_coef_loss, the Polyak step on the critics, and the rewrite of the collection actor's packed weights as in SAC.
 * z, the critics' output deltas and the losses are float64 from float32 operands in one fixed order, each rounded once; no float atomics: the
 * same call on the same state gives the same bits.
 * LIMITS (a message per field otherwise): d_in <= 192, hidden widths 1 .. 256, d_out <= 64, n_critics 1 .. 5, n_quantiles 1 .. 64,
 * n_critics * n_quantiles <= 128, 0 <= top_quantiles_to_drop_per_net <= n_quantiles - 1, 1 <= B <= EV2G_TD3_MAX_BATCH.
 * actor: the 8 host arrays of ev2g_sac_create; critics: 6 per critic, the last layer's [n_quantiles, h2] and [n_quantiles]; float32, [out, in].
 * The object belongs to the handle: freed by ev2g_tqc_destroy or with ev2g_destroy.
 * Not reproduced: use_sde, action_noise, learning_starts, schedule objects (ev2g_tqc_set_rate between calls drives one). */
typedef struct ev2g_tqc ev2g_tqc;
typedef struct ev2g_tqc_config {
    double lr, beta1, beta2, adam_eps, tau, gamma;         /* as ev2g_sac_config: 3e-4, 0.9, 0.999, 1e-8, 0.005, 0.99 */
    double ent_coef;
    double target_entropy;
    int32_t n_critics, target_update_interval;             /* 2, 1 */
    int32_t ent_coef_auto, target_entropy_auto;            /* 1, 1 */
    int32_t n_quantiles, top_quantiles_to_drop_per_net;    /* 25, 2 */
} ev2g_tqc_config;
int ev2g_tqc_default_config(ev2g_tqc_config *cfg);
int ev2g_tqc_create(ev2g_handle *h, const ev2g_tqc_config *cfg, int d_in, int h1, int h2, int d_out, float lo, const float *const *actor,
                    const float *const *critics, uint64_t seed, ev2g_tqc **out);
void ev2g_tqc_destroy(ev2g_handle *h, ev2g_tqc *t);
/* The entries of the SAC section with the same meaning, arguments and staging rules (losses [4]: critic_loss, actor_loss, ent_coef_loss,
 * ent_coef; ev2g_tqc_apply without a pending gradient: EV2G_ERR_STATE).  `out` of get_grads / get_weights: 8 + 6 n_critics arrays. */
int ev2g_tqc_update(ev2g_handle *h, ev2g_tqc *t, const float *obs, const float *actions, const float *reward, const float *next_obs,
                    const uint8_t *done, int B, float *losses);
int ev2g_tqc_critic_grad(ev2g_handle *h, ev2g_tqc *t, const float *obs, const float *actions, const float *reward, const float *next_obs,
                         const uint8_t *done, int B, float *losses);
int ev2g_tqc_actor_grad(ev2g_handle *h, ev2g_tqc *t, const float *obs, int B, float *losses);
int ev2g_tqc_apply(ev2g_handle *h, ev2g_tqc *t);
int ev2g_tqc_act(ev2g_handle *h, ev2g_tqc *t, const float *obs32, int n_rows, int deterministic, float *actions, float *mu, float *log_std,
                 float *log_pi);
int ev2g_tqc_collect(ev2g_handle *h, ev2g_tqc *t, int k_steps, int deterministic, const ev2g_transitions *tr);
int ev2g_tqc_get_grads(ev2g_handle *h, ev2g_tqc *t, float *const *out, float *g_log_ent_coef);
int ev2g_tqc_get_weights(ev2g_handle *h, ev2g_tqc *t, int target, float *const *out);
/* z [B, K] and log pi' [B] (may be NULL) of the last critic gradient (B: its batch size), HOST arrays; synchronises */
int ev2g_tqc_get_z(ev2g_handle *h, ev2g_tqc *t, float *z, float *log_pi_next, int B);
int ev2g_tqc_get_log_pi(ev2g_handle *h, ev2g_tqc *t, float *log_pi, int B);
int ev2g_tqc_get_ent_coef(ev2g_handle *h, ev2g_tqc *t, float *out3);
int ev2g_tqc_set_rate(ev2g_handle *h, ev2g_tqc *t, double lr);
int ev2g_tqc_seed(ev2g_handle *h, ev2g_tqc *t, uint64_t seed, uint64_t first_draw);
int ev2g_tqc_act_seed(ev2g_handle *h, ev2g_tqc *t, uint64_t seed, uint64_t first_launch);
int ev2g_tqc_counters(ev2g_handle *h, ev2g_tqc *t, int64_t *updates, int64_t *target_updates, uint64_t *next_draw, uint64_t *act_launches);
/* The sort-and-truncate kernel alone on the caller's DEVICE arrays: tq [n_critics][B, n_quantiles], log_pi_next, reward [B] float32, done [B]
 * uint8, log_ent_coef one float32; z_out [B, K].  The shape limits above hold.  Asynchronous; a read-only addition for tests, like ev2g_td3_get_y. */
int ev2g_tqc_truncate(ev2g_handle *h, const float *tq, const float *log_pi_next, const float *reward, const uint8_t *done, int B, int n_critics,
                      int n_quantiles, int top_quantiles_to_drop, double gamma, const float *log_ent_coef, float *z_out);
/* Host twins (HOST arrays).  ev2g_host_tqc_target: z [B, K] as ev2g_tqc_truncate forms it (log_ent_coef by value).  ev2g_host_tqc_critic_head:
 * dq [n_critics][B, n_quantiles] and *critic_loss from z [B, K] and q [n_critics][B, n_quantiles], the device's chains and joins. */
int ev2g_host_tqc_target(const float *tq, const float *log_pi_next, const float *reward, const uint8_t *done, int B, int n_critics, int n_quantiles,
                         int top_quantiles_to_drop, double gamma, float log_ent_coef, float *z);
int ev2g_host_tqc_critic_head(const float *z, const float *q, int B, int n_critics, int n_quantiles, int top_quantiles_to_drop, float *dq,
                              float *critic_loss);

/* ---- plain device-memory helpers so a ctypes host needs no other HIP binding --------------- */
void *ev2g_malloc(ev2g_handle *h, size_t bytes);
void ev2g_free(ev2g_handle *h, void *p);
int ev2g_memcpy_h2d(ev2g_handle *h, void *dst, const void *src, size_t bytes);
int ev2g_memcpy_d2h(ev2g_handle *h, void *dst, const void *src, size_t bytes);
/* page-locked host memory (hipHostMalloc) for the buffers a host loop copies every step: the per-step numpy hand-over of the Stable-Baselines3 VecEnv
 * protocol (train_stable_baselines.py:62-130: observations / rewards / dones down, actions up) runs at the PCIe rate from such a buffer, at less than half
 * of it from pageable memory.  Freed by ev2g_host_free or with the handle. */
void *ev2g_host_malloc(ev2g_handle *h, size_t bytes);
void ev2g_host_free(ev2g_handle *h, void *p);
int ev2g_synchronize(ev2g_handle *h);
/* fills [n] doubles with uniform(lo,hi) from a counter-based generator (Philox-free splitmix64
 * keyed on (seed, index)); the same function exists on the host as ev2g_host_uniform so CPU and
 * GPU legs of a benchmark see identical action tensors (RandomAgent, heuristics.py:546-558). */
int ev2g_fill_uniform(ev2g_handle *h, double *dst, int64_t n, uint64_t seed, double lo, double hi);
void ev2g_host_uniform(double *dst, int64_t n, uint64_t seed, double lo, double hi);
/* elapsed GPU time of the kernels enqueued by the last ev2g_step_n(), in milliseconds; total over the K launches.  Measured in one of two ways
 * (ev2g_last_launch_timing says which):
 *   "events"  a pair of HIP events recorded on the handle's stream around the call's launches: the per-step chain, a persistent run cut at the
 *             episode ends, the general kernels, and every other timed entry (ev2g_rollout, ev2g_collect, "timed like ev2g_step_n").
 *   "stamps"  a persistent ev2g_step_n that is ONE launch of ev2g_step_wave's wide stride-0 instantiation (ev2g_last_launch_specialisation 2: the
 *             whole-episode launch of an episode loop) reads the device's constant-rate wall clock (hipDeviceAttributeWallClockRate) itself: the
 *             duration runs from the first workgroup's prologue to the last wavefront's exit.  It does not contain the dispatch ramp in front of
 *             the kernel or the end-of-kernel cache write-back and completion signal behind it, which an event pair includes: a stamped duration
 *             reads 5-6 us shorter than the event pair of the same launch (median 5.2 us at 4096 x 50, 6.0 us at 8192 x 20 PublicPST;
 *             profiles/r28_launch_stamps.txt).  Nothing but the kernel is put on the stream, so the launches
 *             of an episode loop run back to back with the episode-end kernels; an event record between two kernels drains the queue and costs
 *             the loop about 6 us each (profiles/r28_launch_stamps.txt).  Reading a stamped duration waits for the handle's stream.
 * EV2G_LAUNCH_TIMING=events in the environment at load time keeps the event pair on every path. */
double ev2g_last_step_n_kernel_ms(ev2g_handle *h);
/* the same for the timed call `back` calls before the last one (0 = the last; the handle keeps the event pairs or stamp pairs of its last 32
 * ev2g_step_n / ev2g_rollout / ev2g_collect calls): launches can be queued back to back and their durations read afterwards.  -1.0: out of range,
 * a call that failed, or a plain ev2g_step since. */
double ev2g_step_n_kernel_ms_back(ev2g_handle *h, int back);
/* how the last timed call was measured: "stamps", "events", or "" where ev2g_last_step_n_kernel_ms reads -1 */
const char *ev2g_last_launch_timing(const ev2g_handle *h);

/* ---- scenario generator (host side, no GPU involved) ------------------------------------------------------------------
 * What EV2Gym.reset() draws for one episode -- EV sessions (EV_spawner utils.py:477-557, spawn_single_EV :177-345), prices
 * (load_electricity_prices loaders.py:392-461), transformer loads / PV / forecasts / demand-response events
 * (load_transformers loaders.py:227-296, transformer.py:80-256), power setpoints (utils.py:664-757) -- for n_scenarios
 * independent scenarios at once, as an ev2g_scenario_batch ready for ev2g_load_scenarios.  STATISTICALLY matched to the
 * reference (fitted hour-of-day tables and fleet classes; not its CSV data or RNG streams): tests/test_host_logic.py holds it
 * to summary statistics of the reference's own resets.  Every draw is a pure function of (seed, scenario index, counters):
 * the batch does not depend on n_threads, and scenario i of a run with a larger n_scenarios is the same scenario.
 * The fields carry the names and meaning of the YAML keys (ev2gym_env.py:65-166) / of GenConfig in ev2gym_amd/scenario_gen.py. */
typedef struct ev2g_gen_config {
    int32_t simulation_length, timescale;
    int32_t number_of_charging_stations, number_of_ports_per_cs, number_of_transformers;
    int32_t scenario;        /* 0 workplace, 1 public, 2 private                                  */
    int32_t simulation_days; /* 0 weekdays, 1 weekends, 2 both (a uniformly random day of the week) */
    int32_t hour, minute, random_hour;
    int32_t v2g_enabled, power_setpoint_enabled;
    int32_t inflexible_loads, solar_power, demand_response;
    int32_t dr_events_per_day, dr_event_length_minutes_min, dr_event_length_minutes_max, dr_notification_of_event_minutes;
    int32_t heterogeneous_ev_specs, fleet_with_efficiency_tables;
    int32_t fleet;           /* 0 "v2g2024", 1 "ev_plus_phev"                                      */
    int32_t cs_phases, ev_phases, ev_min_time_of_stay;
    int32_t n_ev_specs;      /* > 0: the car models of an EV-specification file replace the built-in fleets (spec_* below) */
    int64_t tr_seed;         /* != -1: loads / PV / events from their own seed (ev2gym_env.py:97-100) */
    double spawn_multiplier, discharge_price_factor, power_setpoint_flexiblity;
    double inflexible_loads_capacity_multiplier_mean, inflexible_loads_forecast_mean, inflexible_loads_forecast_std;
    double solar_power_capacity_multiplier_mean, solar_power_forecast_mean, solar_power_forecast_std;
    double dr_event_capacity_percentage_mean, dr_event_capacity_percentage_std, dr_event_start_hour_mean, dr_event_start_hour_std;
    double transformer_max_power;
    double cs_min_charge_current, cs_max_charge_current, cs_min_discharge_current, cs_max_discharge_current, cs_voltage;
    double ev_battery_capacity, ev_max_ac_charge_power, ev_min_ac_charge_power, ev_max_discharge_power, ev_min_discharge_power;
    double ev_charge_efficiency, ev_discharge_efficiency, ev_transition_soc, ev_transition_soc_multiplier;
    double ev_min_battery_capacity, ev_min_emergency_battery_capacity, ev_desired_capacity;
    /* charging_network_topology file (loaders.py:259-276,312-340), or all NULL: per-charger arrays
       [number_of_charging_stations] and the transformers' max_power [number_of_transformers] */
    const int32_t *topo_n_ports, *topo_transformer, *topo_phases;
    const double *topo_min_charge_current, *topo_max_charge_current, *topo_min_discharge_current, *topo_max_discharge_current;
    const double *topo_voltage, *topo_tr_max_power;
    /* the file `ev_specs_file` names (loaders.py:25-41), or n_ev_specs = 0: per model [n_ev_specs] the registrations (sampling
       weight), battery kWh, max AC charge / discharge kW; spec_efficiency [n_ev_specs][101] percent by charging current in A (the
       nearest-level fill of utils.py:268-288), a row starting with NaN = the model has no table (random scalar efficiency per EV,
       utils.py:290-296); NULL = no model has one */
    const double *spec_registrations, *spec_battery_capacity, *spec_max_ac_charge_power, *spec_max_ac_discharge_power, *spec_efficiency;
    /* tables of an EV2Gym data directory, or all NULL (the fitted hour-of-day tables / synthetic sun curve are used): arrivals per
       port per hour in percent by quarter hour [96] on weekdays / weekend days, mean stay in hours and mean required energy in kWh
       by half hour of arrival [48] (utils.py:199-233,505-528); tab_pv [n_pv] the hourly PV output of a year (loaders.py:165-224) */
    const double *tab_arrival_week, *tab_arrival_weekend, *tab_stay, *tab_energy, *tab_pv;
    int64_t n_pv;
} ev2g_gen_config;
/* fills *cfg with the values of V2GProfitPlusLoads.yaml (kind 0) or PublicPST.yaml (kind 1) */
int ev2g_gen_default_config(int kind, ev2g_gen_config *cfg);
typedef struct ev2g_gen_result ev2g_gen_result;
/* n_threads <= 0: one per hardware thread.  On failure returns a negative code, *out = NULL (ev2g_last_error(NULL) says why). */
int ev2g_generate(const ev2g_gen_config *cfg, int32_t n_scenarios, uint64_t seed, int32_t n_threads, ev2g_gen_result **out);
const ev2g_scenario_batch *ev2g_gen_batch(const ev2g_gen_result *r); /* arrays owned by r */
void ev2g_gen_free(ev2g_gen_result *r);
/* ---- scenario generation ON THE DEVICE: new scenarios drawn straight into the resident pool ------------------------------
 * EV2Gym.reset() draws a new scenario every episode (ev2gym_env.py:243-296).  The resident pool gives every episode fresh scenarios
 * for pool / envs episodes; this call re-draws pool slots [first_slot, first_slot + n) WITHOUT host work or PCIe traffic: slot
 * first_slot + j becomes scenario first_index + j of the stream (cfg, seed) -- bit for bit what ev2g_generate(cfg, ., seed) yields at
 * that index followed by ev2g_load_scenarios (one wavefront per scenario runs the generator's own code, csrc/ev2g_refill.h).
 * Requirements: the pool was loaded with EV2G_FLAG_REFILLABLE from a batch drawn with the same config (shape, fleet, topology).  Chargers
 * with several ports and charging_network_topology files are supported up to 256 steps and 256 ports (the kernel replays the reference's
 * first-free port assignment, ev_charger.py:266-286, per charger; a generator port that draws more than 8 sessions is cut and counted as an
 * overflow).  Asynchronous on the handle's stream; refill slots that no env is currently stepping (e.g. the window
 * the previous episode used).  Afterwards ev2g_peek is refused (the host holds no copy of the new scenarios).
 * ev2g_pool_refill_overflows: scenarios (since load) that drew more sessions than ev2g_pool_session_capacity slots and were
 * truncated (synchronises; 0 in practice: the blocks are 25 % + 8 larger than the largest scenario of the loaded batch). */
int ev2g_pool_refill(ev2g_handle *h, const ev2g_gen_config *cfg, uint64_t seed, int64_t first_index, int32_t first_slot, int32_t n);
long long ev2g_pool_refill_overflows(ev2g_handle *h);
int ev2g_pool_session_capacity(const ev2g_handle *h);
/* the generator's fitted tables: which = 0 arrivals per port per hour in percent, 1 mean stay in hours (24 values each),
 * 2 mean required energy (1 value), for table kind 0 workplace, 1 public, 2 private, 3 public weekend, 4 private weekend;
 * which = 3 / 4: the V2G / EV+PHEV fleet as rows of (share, battery kWh, max AC kW); returns the number of values written */
int ev2g_gen_table(int which, int kind, double *out, int n_max);

/* ---- ARS on the device: sb3_contrib's ARS (Augmented Random Search) with per-candidate weights (csrc/ev2g_ars.h, ev2g_ars_host.h) ----
 *   MlpPolicy (EV2G_ARS_MLP):       obs -> ReLU(h1) -> ReLU(h2) -> linear(d_out) -> tanh, unscaled into the env's box [lo, 1]; theta = W1 | b1 | W2 | b2 | W3 | b3
 *   LinearPolicy (EV2G_ARS_LINEAR): obs -> linear(d_out), no bias, clipped to [lo, 1] (h1, h2 are not read);                   theta = W
 * every matrix [out, in] row-major (parameters_to_vector).  One iteration: ev2g_ars_perturb draws delta [n_delta, n_params] ~ N(0, 1) -- direction
 * k's element i of iteration n is draw (n n_delta + k) n_params + i of ev2g_ac_host_normal's generator under the object's seed -- and writes the
 * 2 n_delta candidates' packed weights (k: theta + delta_std delta_k, n_delta + k: theta - delta_std delta_k, float32, each operation rounded
 * once); the population actor evaluates n_rows = C R rows as C = 2 n_delta candidates of R consecutive rows, each under ITS OWN weights, in one
 * launch; ev2g_ars_rollout in population mode steps the engine's envs under it and sums every env's rewards (float64, steps ascending); ev2g_ars_update forms
 * return[c] = sum of candidate c's envs ascending + alive_bonus_offset x the steps they took, ranks score_k = max(r+_k, r-_k) descending (ties to
 * the lower k), keeps n_top directions, sigma_R = their 2 n_top returns' unbiased standard deviation (r+ in rank order, then r-),
 * step = learning_rate / (n_top sigma_R + 1e-6), theta_i <- (float)(theta_i + step sum_j (r+_j - r-_j) delta_j,i) in float64, j in rank order.
 * A return that is not finite refuses the update inside the launch: theta keeps its bits and the report says which candidate.  Everything is
 * queued on the handle's stream with device-resident state; sums run in one fixed order, no atomics: the same calls give the same bits, and
 * the host twins below give the device's bits.  A row's action depends on its candidate's weights alone, not on R, C or the row's place.
 * LIMITS (a message per field otherwise): d_in <= 192, hidden widths 1 .. 256, d_out <= 64, 1 <= n_top <= n_delta <= 4096.
 * The object belongs to the handle: freed by ev2g_ars_destroy or with ev2g_destroy. */
#define EV2G_ARS_MLP 0
#define EV2G_ARS_LINEAR 1
typedef struct ev2g_ars ev2g_ars;
typedef struct ev2g_ars_config {
    double learning_rate, delta_std, alive_bonus_offset;   /* 0.02, 0.05, 0 */
    int32_t n_delta, n_top;                                /* 8, 8 */
} ev2g_ars_config;
typedef struct ev2g_ars_info {
    int32_t max_in, max_hidden, max_out, max_delta;        /* the limits */
    int32_t n_params;
    int64_t candidate_floats;                              /* one candidate's packed image */
    int64_t image_bytes, delta_bytes, total_bytes;         /* 1 + 2 n_delta images; the directions; everything the object allocates at create */
    int64_t lds_bytes;                                     /* of the population actor's workgroup */
} ev2g_ars_info;
typedef struct ev2g_ars_report {
    double sigma_r, step;
    int64_t iteration;                                     /* the iteration whose directions the update used */
    int32_t refused, first_bad, n_top;                     /* refused != 0: first_bad is the first candidate whose return was not finite (else -1) */
    int32_t reserved;
} ev2g_ars_report;
int ev2g_ars_default_config(ev2g_ars_config *cfg);
/* what an object of this shape takes; a refused shape or config returns the code, ev2g_last_error(NULL) the message */
int ev2g_ars_query(const ev2g_ars_config *cfg, int kind, int d_in, int h1, int h2, int d_out, ev2g_ars_info *out);
/* theta: HOST float32 [n_params], or NULL for zeros (sb3_contrib's zero_policy) */
int ev2g_ars_create(ev2g_handle *h, const ev2g_ars_config *cfg, int kind, int d_in, int h1, int h2, int d_out, float lo, const float *theta,
                    uint64_t seed, ev2g_ars **out);
void ev2g_ars_destroy(ev2g_handle *h, ev2g_ars *a);
/* the next iteration's directions and candidate weights; zeroes the envs' returns and the step count; the iteration counter advances */
int ev2g_ars_perturb(ev2g_handle *h, ev2g_ars *a);
/* DEVICE obs32 [n_rows, d_in] -> actions [n_rows, d_out] in [lo, 1].  population == 0: every row under theta; else n_rows must be a positive
 * multiple of 2 n_delta and rows [c R, (c + 1) R) run under candidate c (after an ev2g_ars_perturb). */
int ev2g_ars_act(ev2g_handle *h, ev2g_ars *a, const float *obs32, int n_rows, int population, float *actions);
/* The object's own float32 observation row [E, D] and action row [E, P] (allocated on first use): ev2g_reset_f32 into the first one starts an
 * episode for ev2g_ars_rollout, which keeps it current. */
float *ev2g_ars_obs_f32(ev2g_handle *h, ev2g_ars *a);
float *ev2g_ars_actions_f32(ev2g_handle *h, ev2g_ars *a);
/* k_steps x (population or centre actor on the object's observation row -> one-step launch), a segment inside one episode; the rows reward
 * [k_steps, r_stride >= E] DEVICE float64 are kept when given, in both modes.  population != 0: then every env's rewards are added to its return
 * and the steps counted.  population == 0 (an evaluation of theta) is no part of the iteration: it changes neither the envs' returns nor the step
 * count, so it may stand anywhere between ev2g_ars_perturb and ev2g_ars_update.  On the fast path the step reads
 * and writes the object's rows per launch; elsewhere through the registered float32 hand-over buffers (ev2g_set_step_extras, observation
 * stride 0), as ev2g_ac_collect.  population != 0: E must be a positive multiple of 2 n_delta.  No link, grid or wrapper is applied. */
int ev2g_ars_rollout(ev2g_handle *h, ev2g_ars *a, int k_steps, int population, double *reward, int64_t r_stride);
/* the step from the envs' returns of the rollouts since the last perturb, or from ev2g_ars_set_returns' */
int ev2g_ars_update(ev2g_handle *h, ev2g_ars *a);
/* HOST read-backs; all synchronise; each out may be NULL.  returns [2 n_delta] float64, ranks [n_delta] (direction k's rank, 0 the best) */
int ev2g_ars_get_report(ev2g_handle *h, ev2g_ars *a, ev2g_ars_report *report, double *returns, int32_t *ranks);
int ev2g_ars_get_weights(ev2g_handle *h, ev2g_ars *a, float *theta);
int ev2g_ars_set_weights(ev2g_handle *h, ev2g_ars *a, const float *theta);
/* candidate c's parameter vector [n_params], unpacked from its image */
int ev2g_ars_get_candidate(ev2g_handle *h, ev2g_ars *a, int c, float *theta);
int ev2g_ars_get_deltas(ev2g_handle *h, ev2g_ars *a, float *delta);
int ev2g_ars_get_env_returns(ev2g_handle *h, ev2g_ars *a, double *env_return, int n_envs);
/* 2 n_delta HOST returns in front of the next update, in place of the envs' */
int ev2g_ars_set_returns(ev2g_handle *h, ev2g_ars *a, const double *returns);
int ev2g_ars_set_rates(ev2g_handle *h, ev2g_ars *a, double learning_rate, double delta_std);
int ev2g_ars_seed(ev2g_handle *h, ev2g_ars *a, uint64_t seed, uint64_t first_iteration);
/* the next perturb's iteration, updates queued, env steps since the last perturb (each may be NULL) */
int ev2g_ars_counters(ev2g_handle *h, ev2g_ars *a, uint64_t *next_iteration, int64_t *updates, int64_t *steps);
/* Host twins (HOST arrays), bit for bit what the launches compute.  perturb: delta [n_delta, n_params] and cand [2 n_delta, n_params] (may be
 * NULL) of iteration n.  returns: env_return [n_envs] += the rows reward [k, r_stride] (NULL: nothing), then returns [n_candidates] (may be NULL)
 * of n_envs / n_candidates consecutive envs each.  update: theta [n_params] in place, ranks [n_delta], the report. */
int ev2g_host_ars_perturb(const float *theta, int n_delta, int n_params, double delta_std, uint64_t seed, uint64_t iteration, float *delta, float *cand);
int ev2g_host_ars_returns(double *env_return, const double *reward, int k, int64_t r_stride, int n_envs, int n_candidates, double alive_bonus_offset,
                          int64_t steps, double *returns);
int ev2g_host_ars_update(float *theta, const float *delta, const double *returns, int n_delta, int n_top, int n_params, double learning_rate,
                         int32_t *ranks, ev2g_ars_report *report);

#ifdef __cplusplus
}
#endif
#endif /* EV2G_H */
