// ev2g_host.hip -- host side of libev2g_hip.so: the C-ABI of include/ev2g.h over HIP.
//
// Scenario packing turns the reference-shaped batch (chargers, transformers, EVs_profiles-ordered sessions) into the device
// layout documented in ev2g_device.h / DESIGN.md.  Its host half -- transformer-major port slots, sessions sorted by
// (env, slot, arrival) with the next session's window chained in, per-port first-session tables, max_energy_AFAP -- is
// ev2g_load_host.h's LoadPlan; ev2g_load_scenarios below routes, uploads and allocates (its load_* functions).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <array>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ev2g.h"
#include "ev2g_device.h"
#include "ev2g_load_host.h"
#include "ev2g_route_host.h"
#include "ev2g_balance_host.h"
#include "ev2g_timing_host.h"
#include "ev2g_policy_host.h"
#include "ev2g_step_v2.h"
#include "ev2g_step_wave.h"
#include "ev2g_step_big.h"
#include "ev2g_mlp.h"
#include "ev2g_comm.h"
#include "ev2g_refill.h"
#include "ev2g_heuristic.h"
#include "ev2g_link.h"
#include "ev2g_grid.h"
#include "ev2g_wrap.h"
#include "ev2g_ac.h"
#include "ev2g_ppo.h"
#include "ev2g_learner_host.h"
#include "ev2g_trpo_host.h"
#include "ev2g_td3_host.h"
#include "ev2g_sac_host.h"
#include "ev2g_tqc_host.h"
#include "ev2g_ars.h"
#include <cstdlib>

static thread_local std::string g_create_error;
#include "ev2g_gen_host.h"

// What every object a handle owns (and ev2g_destroy, a destroy entry or a failed create releases) keeps of its device memory: each block
// is allocated into one of the two pools with `upload` / `dalloc`, and release_owned frees the pools.  The named pointers of an object are
// what the kernels' argument structs are filled from, not a record of ownership.
struct DevOwner {
    std::vector<void *> allocs;        // the blocks of create, and those allocated on first use: kept for the object's life
    std::vector<void *> swap_allocs;   // the blocks a later call drops and refills as a whole (a grid's attached state, a policy's clipped block)
};

// a queue of ports per env, the RoundRobin agents' and Rescale_RepairLayer's (queue_alloc): the entries, each env's length and, where the kind
// keeps them, every entry's min_power / max_power
struct PortQueue {
    int *queue = nullptr, *qlen = nullptr;   // [E, P], [E]
    double *qmin = nullptr, *qmax = nullptr; // [E, P] each, or nullptr
};

// an env-reading heuristic agent on the device (ev2g_heuristic_create): its kind, the shape it was made for, the RoundRobin agents' queues
// (RoundRobin_GF*: with every entry's min_power / max_power) and the action block ev2g_heuristic_run writes when the caller passes none
struct ev2g_heuristic : DevOwner {
    int kind = 0, E = 0, P = 0;
    PortQueue q;
    double *act = nullptr;                   // [E, P]
};

// a communication-fault link (ev2g_link_create, ev2g_link.h): the two probabilities, the uniforms of each half (a [T, E, P] device matrix, or
// the seed of the generated ones), the shape it was made for, the held commands (FailedActionCommunication.previous_actions_list) and the two
// remembered energy columns (DelayedObservation.previous_obs_list / actual_previous_obs_list, column 4 + 3 i), and the blocks ev2g_link_run /
// ev2g_link_rollout work on when the caller passes none (allocated on first use)
struct ev2g_link : DevOwner {
    int E = 0, P = 0, T = 0;
    double p_fail = 0.0, p_delay = 0.0;
    unsigned long long seed_act = 0, seed_obs = 0;
    double *rand_act = nullptr, *rand_obs = nullptr;   // [T, E, P] each, or nullptr
    double *held = nullptr, *prev = nullptr, *actual = nullptr;   // [E, P] each
    double *raw = nullptr, *obs = nullptr;             // [E, P] the agent's raw actions, [E, D] the observation row
    float *obs32 = nullptr, *act32 = nullptr;          // [E, D], [E, P]: the policy's input and output rows
};

// a distribution grid (ev2g_grid_create, ev2g_grid.h): the network's K (transposed) and L, the solver's settings, the base profiles of every
// resident scenario when the grid was made for ev2g_grid_run, the shape it was made for, and the per-env rows ev2g_grid_run works on when the
// caller passes none
struct ev2g_grid : DevOwner {
    int E = 0, T = 0, M = 0, n = 0, max_iter = 0;
    double s_base = 0.0, tolerance = 0.0;
    double2 *Kt = nullptr, *L = nullptr;            // [n, n], [n]
    double *p_base = nullptr, *q_base = nullptr;    // [M, T + 1, n] each, or nullptr: a solver only
    double *vm = nullptr, *rew = nullptr;           // [E, n + 1], [E]
    // the episode's voltage statistics (ev2g_grid_kernel<true>'s accumulators), with profiles only: [E] each
    double *vv_sum = nullptr, *rew_sum = nullptr;
    int *vv_count = nullptr, *vv_steps = nullptr;
    // V2G_grid_state (ev2g_grid_state_attach, in swap_allocs): the time-feature table [M or 1, T + 1, 3], the row width 6 + 2 n + 3 P, the grid's
    // own rows [E, Dg] and the blocks ev2g_grid_rollout works on ([E, P] each); obs32 holds the state of step counter obs32_step as long as
    // nothing has changed the engine's state since (obs32_epoch == the handle's state_epoch), -1: nothing
    double *tf = nullptr;
    int tf_per_scn = 0, Dg = 0;
    double *obs = nullptr, *act = nullptr;
    float *obs32 = nullptr, *act32 = nullptr;
    int obs32_step = -1;
    long long obs32_epoch = -1;
};

// an action wrapper (ev2g_wrap_create, ev2g_wrap.h): its kind, the shape it was made for, Rescale_RepairLayer's queue of every env with each
// entry's min_power / max_power, and the float64 block the step reads when the caller passes no `wrapped` rows
struct ev2g_wrap : DevOwner {
    int kind = 0, E = 0, P = 0;
    PortQueue q;
    double *act = nullptr;                   // [E, P]
};

// a Gaussian actor-critic (ev2g_ac_create, ev2g_ac.h): the packed network, the noise stream's seed and launch counter, and the clipped action
// block [E, P] the step of ev2g_ac_collect reads (in swap_allocs: allocated on first use, regrown when E * P grows)
struct ev2g_acpolicy : DevOwner {
    AcDev dev{};
    AcPlan plan{};   // the padded sizes the weight images are packed for (ev2g_policy_host.h)
    size_t lds = 0;
    int relu = 0;
    unsigned long long seed = 0, n = 0;
    float *clipped = nullptr;
    size_t clipped_elems = 0;
    std::vector<float> log_std;           // the values last uploaded (ev2g_ac_get_weights returns them when no learner is bound)
    struct ev2g_ppo *learner = nullptr;   // the learner bound to this policy (ev2g_ppo_create / ev2g_a2c_create), destroyed with it
};

// the learner of an actor-critic (ev2g_ppo_create / ev2g_a2c_create, ev2g_ppo.h): float32 masters of the thirteen arrays in SB3's layout with
// the optimiser's state (Adam's m and v; RMSprop's square average in v), the gradient of the last grad call, the transposed images backprop
// reads, and the gradient kernel's workspace
static_assert(LEARNER_HEAD_PPO == EV2G_HEAD_PPO && LEARNER_HEAD_A2C == EV2G_HEAD_A2C, "LearnerSpec::head is ev2g_ppo_grad_kernel's HEAD");
struct ev2g_ppo : DevOwner {
    LearnerSpec spec;          // kind, head, hyper-parameters, optimiser (ev2g_learner_host.h)
    ev2g_acpolicy *ac = nullptr;
    PpoPlan plan;
    float *theta = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *work = nullptr;
    double *stat_part = nullptr, *norm_part = nullptr, *advstat = nullptr;
    PpoDev dev{};
    PpoMap map{};
    int n_blocks = 0;          // blocks of the reduce / apply launches: ceil(n_params / 256)
    long long t = 0;           // the optimiser's step count
    bool have_grad = false;    // a gradient no apply has consumed yet
    // a TRPO learner (ev2g_trpo_create, ev2g_trpo.h): its config, the solve's float64 vectors and theta0 [n_actor], the direction images, the
    // step's state, the per-workgroup partials, and mu0 [B, P] (in swap_allocs: regrown when B * P grows)
    TrpoSpec trpo;
    TrpoPlan tplan;
    TrpoMap tmap{};
    double *tg = nullptr, *tx = nullptr, *tr = nullptr, *tp = nullptr, *thv = nullptr, *tpart = nullptr;
    float *theta0 = nullptr, *mu0 = nullptr, *dimg[EV2G_TRPO_ACTOR_ARRAYS] = {};
    TrpoState *tstate = nullptr;
    size_t mu0_elems = 0;
    int n_ablocks = 0;         // blocks of the launches over a flat actor vector
    bool have_step = false;    // a policy step was queued: there is a report and a direction
};

// the TD3 / DDPG learner of a policy (ev2g_td3_create, ev2g_td3.h): float32 masters, targets, Adam's state and the last gradient in the plan's
// flat layout (actor | critic 0 | critic 1), the workspace of one batch, the two losses, and the map its refresh writes the policy's images by
struct ev2g_mlp;
struct ev2g_td3 : DevOwner {
    ev2g_td3_config cfg{};
    ev2g_mlp *policy = nullptr;
    Td3Plan plan;
    MlpImageMap map{};
    float lo = -1.0f;
    float *theta = nullptr, *target = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *work = nullptr, *loss = nullptr;
    unsigned long long seed = 0, next_draw = 0;
    long long n = 0, t_critic = 0, t_actor = 0;   // updates applied to the critics; Adam's step counts
    int pending = 0, last_B = 0;                  // gradients no apply has consumed yet (bit 0: the critics', bit 1: the actor's); the batch size of the last critic gradient
};
static void td3_free(ev2g_td3 *t);

// What a SAC learner and a TQC learner share -- each with its collection actor (ev2g_sac_create / ev2g_tqc_create, ev2g_sac.h): float32 masters,
// Adam's state and the last gradient in the plan's flat layout (actor | critic 0 | critic 1 | ...), the target critics, log_ent_coef with its Adam
// state and gradient, the workspace of one batch, the four losses, the collection actor's packed images, and the two noise streams.  `abi` is
// the prefix of the object's entries ("ev2g_sac" / "ev2g_tqc"): what the shared stages' messages name.
struct SacCore : DevOwner {
    const char *abi = "ev2g_sac";
    ev2g_sac_config cfg{};
    SacPlan plan;
    SacDev dev{};
    size_t lds = 0;
    float lo = -1.0f;
    double target_entropy = 0.0;
    float *theta = nullptr, *target = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *work = nullptr, *loss = nullptr;
    float *alpha = nullptr, *g_alpha = nullptr;   // {log_ent_coef, m, v}; its gradient
    unsigned long long seed = 0, next_draw = 0, act_seed = 0, act_n = 0;
    long long n = 0, n_target = 0, t_critic = 0, t_actor = 0;   // updates applied, Polyak steps among them; Adam's step counts
    int pending = 0, last_B = 0, last_actor_B = 0;              // bit 0: the critics' gradient, bit 1: the actor's and log_ent_coef's
};
struct ev2g_sac : SacCore {};
// a TQC learner (ev2g_tqc_create, ev2g_tqc.h): SacCore with quantile critics -- `plan` is tq's SacPlan part (q, tq, dq as [nc][B, nq]), tq adds z,
// the rows' float64 partials and the summed input deltas
struct ev2g_tqc : SacCore {
    TqcPlan tq;
};

// an ARS learner (ev2g_ars_create, ev2g_ars.h): theta, the centre image and the 2 n_delta candidate images, the directions of the last perturb,
// the envs' returns (regrown with E, in swap_allocs, with the object's observation, action, reward, done and mask rows), the candidates' returns, the ranks
// and the report; what the host knows of an iteration's progress
struct ev2g_ars : DevOwner {
    ev2g_ars_config cfg{};
    ArsPlan plan;
    ArsDev dev{};
    float *theta = nullptr, *centre = nullptr, *cand = nullptr, *delta = nullptr;
    double *ret = nullptr, *env_return = nullptr, *reward = nullptr;
    int32_t *rank = nullptr, *order = nullptr;
    ev2g_ars_report *report = nullptr;
    float *obs32 = nullptr, *act32 = nullptr;
    uint8_t *done = nullptr, *mask = nullptr;   // [E], [E, P]: every step's, overwritten (the full step instantiation writes all its outputs)
    long long rows_E = 0, rows_D = 0, rows_P = 0, rows_T = 0;   // what the swap blocks were sized for
    unsigned long long seed = 0, iter = 0;   // the next perturb's iteration
    long long updates = 0, steps = 0;        // updates queued; env steps since the last perturb
    int roll_E = 0;                          // the envs of the rollouts since the last perturb (0: none)
    bool have_dirs = false, returns_set = false;
};

#define EV2G_EV_RING TIMING_RING
struct ev2g_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    ev2g_config cfg{};
    bool loaded = false;
    DevScn scn{};
    DevState st{};
    std::vector<void *> scn_allocs, st_allocs, user_allocs;
    std::vector<void *> user_host_allocs;       // ev2g_host_malloc: page-locked host buffers of the caller's per-step copies
    void *peek_stage = nullptr; size_t peek_stage_bytes = 0;   // ev2g_peek's page-locked staging block
    // host mirrors for peek / stats
    int E = 0, M = 0, T = 0, C = 0, npc = 0, P = 0, R = 0, D = 0;   // E envs stepped concurrently, M scenarios in the pool
    long long scn_off = 0;                      // env e runs scenario (e + scn_off) mod M
    ev2g_step_extras extras{};
    long long S = 0;
    std::vector<int> slot_port, port_slot;
    std::vector<long long> env_sess_start;      // [E+1] host order
    std::vector<int> host_to_dev;               // [S] device session index of host session
    std::vector<int> sess_port;                 // [S] resolved reference port, host order
    std::vector<double> sess_afap;              // [S] host order
    long long *d_env_sess = nullptr;            // unused placeholder for the stats kernel signature
    double *d_ss_afap = nullptr;                // [S] device order
    double *d_step_tab = nullptr;               // [M,T,8] (fast path)
    V2P *d_v2p = nullptr;                       // device copy of the v2 kernel's parameter block
    double *d_head_tab = nullptr; int head_nh = 0;   // observation head table of the fast path (rebuilt for refilled slots)
    double *d_lut_rowmax = nullptr;             // [n_lut] largest entry of every efficiency table
    bool refilled = false;                      // ev2g_pool_refill ran: the host copies of the scenarios (peek) no longer describe the pool
    int *d_refill_overflow = nullptr;
    struct RefillCache {                        // device copies of the generator config's arrays, kept while the config does not change
        std::vector<unsigned char> key;
        std::vector<void *> allocs;
        RefillArgs args{};
    } refill_cache;
    int sess_cap = 0;                           // EV2G_FLAG_REFILLABLE: session slots per scenario of the resident pool (0: packed storage)
    // a launch's route (ev2g_route_host.h): what the load fixed of it, and what route_step made of the last step launch (launch_fused: 4) --
    // the reporters and launch_stats read `last`; every call that changes the envs' state discards its in-launch statistics
    RouteShape shape;
    StepRoute last;
    std::string big_reason;                     // why ev2g_step_big does not take the launches ev2g_step_v2<1024, 1> would ("" when it does / when the shape is not a big env)
    size_t lds_big = 0;
    BigArgs big_args{};
    // battery-maths dictionary (ClsRec, ev2g_device.h): host mirror of the entries in use, so that ev2g_pool_refill can append the
    // classes its fleet may draw; d_cls_rec has room for EV2G_CLS_CAP entries when DevScn::dict is set
    std::map<ClsKey, int> cls_map;
    ClsRec *d_cls_rec = nullptr;
    std::vector<double> cs_vk_host;             // [C,4] voltage*sqrt(k) and [C] phases of the loaded chargers (the refill's dictionary entries)
    std::vector<int> cs_ph_host;
    std::vector<double> cs_imax_host;           // [C] max_charge_current of the loaded chargers: only so that the refill can call ev2g_sess_consts, the one
                                                // place the record constants are formed (the potc it yields is not part of a dictionary entry: ev2g_cls_of)
    int load_gen = 0;                           // counts ev2g_load_scenarios calls (part of the refill cache's key)
    // in-launch episode statistics (ev2g_step_wave's INL phase): the last step launch closed the episode and wrote get_statistics of every env
    // into d_stats_inl; ev2g_get_stats / ev2g_get_stats_reset copy those rows while nothing has changed the state since (every state-changing
    // call clears the flag).  EV2G_NO_INLAUNCH_STATS=1 at load time: every episode end runs ev2g_stats_kernel (A/B, parity tests)
    double *d_stats_inl = nullptr;              // [E, EV2G_N_STATS]: the loaded shape has the in-launch phase (V2P::stats_inl points here), else nullptr
    // fast-forward of EV-free stretches (ev2g_step_wave's FFW path): per-workgroup counts of the last eligible launch; EV2G_NO_FAST_FORWARD=1 at load
    // time leaves the block (and V2P::ff_count) null, and every step is stepped (A/B, parity tests)
    unsigned long long *d_ff_count = nullptr;   // [n_groups]
    unsigned *d_place = nullptr;                // [2 * n_groups + 2048] V2P::place (EV2G_PLACEMENT=1 at load time, development), else null
    // CU balance (ev2g_balance_host.h): every scenario's live-step bitset (host, from the sessions' windows at load) and the maps made from them, one
    // per pool window a launch started on -- a window's map depends on nothing but the pool and the offset, so it is built once and kept on the device
    struct BalanceMap { long long off; int moved; std::vector<int> host; };   // (host: what was uploaded; slot i of d_balance holds maps[i])
    std::vector<uint64_t> balance_bits;         // [M][BALANCE_WORDS]
    std::vector<BalanceMap> balance_maps;       // at most kBalanceSlots, then the oldest slot is rebuilt
    int *d_balance = nullptr;                   // [kBalanceSlots][n_groups]
    size_t balance_next = 0;                    // the slot the next new window takes
    int balance_cus = 0;                        // the device's CU count
    int last_balance_moved = 0;                 // ev2g_last_launch_balance
    int last_stats_route = -1;                  // ev2g_last_stats_route
    const char *stats_reason = "";              // ev2g_last_stats_reason: last.inl_reason at the last ev2g_get_stats / ev2g_get_stats_reset
    std::string kernel_name;                    // the step kernel ev2g_load_scenarios selected (ev2g_kernel_name)
    std::string fallback_reason;                // why the common-shape fast path was NOT taken ("" when it was / does not apply)
    int current_step = 0;
    long long state_epoch = 0;                  // counts the calls that change the envs' state (load, reset, step launches, refill): what a grid's obs32 row is valid for
    size_t lds_bytes = 0;
    // HIP-event pairs of the last EV2G_EV_RING timed calls (timed_open / timed_close: ev2g_step_n, ev2g_rollout, ev2g_collect and run_chain's
    // callers -- ev2g_heuristic_run, ev2g_link_run / _rollout, ev2g_grid_run / _run_observed / _rollout; not ev2g_step): a caller that queues
    // several launches and reads their durations afterwards (bench.py's roofline pass) does not have to drain the stream after each one
    hipEvent_t ev0s[EV2G_EV_RING] = {}, ev1s[EV2G_EV_RING] = {};
    // the ring's bookkeeping (ev2g_timing_host.h).  A persistent ev2g_step_n that is ONE launch of ev2g_step_wave is timed by the kernel's own clock
    // stamps (the wide stride-0 instantiations: StepRoute::stamps) instead of an event pair -- slot i's pair is d_stamps[2 i], [2 i + 1] --, so that nothing but kernels stands on the stream between the
    // launches of an episode loop; EV2G_LAUNCH_TIMING=events at load time keeps the event pair everywhere
    TimingRing ring;
    unsigned long long *d_stamps = nullptr;     // [EV2G_EV_RING][2], zeroed at creation, freed with the handle (life_allocs)
    std::vector<void *> life_allocs;            // device blocks that live as long as the handle
    int wall_khz = 0;                           // hipDeviceAttributeWallClockRate of the handle's device (0: unknown -- no stamps)
    bool timing_events = false;                 // LoadSwitches::timing_events of the last load
    unsigned fused_attr_mask = 0;               // fused instantiations whose dynamic-LDS attribute was set for THIS handle's device (bit = FusedRoute::index)
    std::string err;
    CommState comm;                             // RCCL communicator of the statistics exchange (ev2g_comm_init), if any
    // ev2g_rollout segments captured as HIP graphs: a policy-in-the-loop step is two short dependent kernels, so the enqueue cost
    // of 2k launches (and the gaps between them) is comparable to the kernels; a segment with the same signature is replayed
    struct RolloutGraph {
        const void *mlp; int k, t0; long long scn_off; const void *rew, *done, *mask; long long rs, ds, ms;
        ev2g_step_extras x; hipGraphExec_t exec;
    };
    std::vector<RolloutGraph> rollout_graphs;
    long long graph_launches = 0;
    // the env-reading heuristic agents (ev2g_heuristic.h): port -> slot table and the charger constants in the reference's operation
    // order (rebuilt by every load), and the agents created on this handle (freed with it)
    int *d_port_slot = nullptr;
    double *d_heur_cs_kw = nullptr, *d_heur_cs_min_kw = nullptr;
    double heur_avg_power = 0.0, heur_min_action = 0.0;
    std::vector<ev2g_heuristic *> heuristics;
    std::vector<ev2g_link *> links;             // the communication-fault links created on this handle (freed with it)
    std::vector<ev2g_grid *> grids;             // the distribution grids created on this handle (freed with it)
    std::vector<ev2g_wrap *> wraps;             // the action wrappers created on this handle (freed with it)
    std::vector<ev2g_acpolicy *> acs;           // the Gaussian actor-critics created on this handle (freed with it)
    std::vector<ev2g_ppo *> ppos;               // the learners (PPO and A2C) created on this handle (freed with it, or with their policy)
    std::vector<ev2g_td3 *> td3s;               // the TD3 / DDPG learners created on this handle (freed with it, or with their policy)
    std::vector<ev2g_sac *> sacs;               // the SAC learners created on this handle (freed with it)
    std::vector<ev2g_tqc *> tqcs;               // the TQC learners created on this handle (freed with it)
    std::vector<ev2g_ars *> arss;               // the ARS learners created on this handle (freed with it)
    unsigned ars_attr_mask = 0;                 // ev2g_ars_act_kernel instantiations (bit kind) whose dynamic-LDS attribute was set for this handle's device
    unsigned sac_attr_mask = 0;                 // ev2g_sac_act_kernel instantiations whose dynamic-LDS attribute was set for this handle's device
    unsigned trpo_attr_mask = 0;                // the TRPO kernels likewise (bit relu)
    unsigned ppo_attr_mask = 0;               // ev2g_ppo_grad_kernel instantiations (bit relu + 2 head) whose dynamic-LDS attribute was set
    unsigned ac_attr_mask = 0;                  // ev2g_ac_act_kernel instantiations whose dynamic-LDS attribute was set for this handle's device
};

#define HIPCHK(h, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
            return EV2G_ERR_HIP;                                                                     \
        }                                                                                            \
    } while (0)

static int fail(ev2g_handle *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    else g_create_error = msg;
    return code;
}

template <typename T>
static int upload(ev2g_handle *h, std::vector<void *> &pool, const T *src, size_t n, T **dst) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIPCHK(h, hipMalloc(&p, bytes));
    pool.push_back(p);
    if (n) HIPCHK(h, hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    *dst = (T *)p;
    return 0;
}
template <typename T>
static int dalloc(ev2g_handle *h, std::vector<void *> &pool, size_t n, T **dst) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIPCHK(h, hipMalloc(&p, bytes));
    HIPCHK(h, hipMemsetAsync(p, 0, bytes, h->stream));
    pool.push_back(p);
    *dst = (T *)p;
    return 0;
}
// every call that changes the envs' state: the last launch's in-launch statistics are no longer those of the state (`why`: what
// ev2g_last_stats_reason reports), and a grid's float32 row is stale
static void state_changed(ev2g_handle *h, const char *why) {
    h->last.inl_stats = false; h->last.inl_reason = why; h->state_epoch += 1;
}

// waits for everything queued on the handle's stream: what a call does before host memory that queued copies read goes away
static int drain(ev2g_handle *h) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

static void free_pool(std::vector<void *> &pool) {
    for (void *p : pool) (void)hipFree(p);
    pool.clear();
}

// The bracket of a timed call: timed_open takes the next slot of the event ring once the arguments are accepted, timed_close records the end
// on the success path only -- a call that returns an error in between leaves the slot invalid (its duration reads -1) and `timed` as it was.
// A call that knows only behind route_step what it launches (ev2g_step_n's single persistent launch) takes the slot first and lets launch_steps
// decide between timed_events and timed_stamps; every other call is timed_open = slot + opening event.
static int timed_events(ev2g_handle *h) {
    h->ring.open(TIMING_EVENTS);
    HIPCHK(h, hipEventRecord(h->ev0s[h->ring.slot], h->stream));
    return EV2G_OK;
}
static bool stamps_usable(const ev2g_handle *h) { return h->d_stamps != nullptr && h->wall_khz > 0 && !h->timing_events; }
static unsigned long long *timed_stamps(ev2g_handle *h) {   // the slot's pair, for WaveArgs::stamp
    h->ring.open(TIMING_STAMPS);
    return h->d_stamps + 2 * (size_t)h->ring.slot;
}
static int timed_open(ev2g_handle *h) {
    h->ring.take();
    return timed_events(h);
}
static int timed_close(ev2g_handle *h) {
    if (h->ring.kind[h->ring.slot] == TIMING_EVENTS) HIPCHK(h, hipEventRecord(h->ev1s[h->ring.slot], h->stream));
    h->ring.close();
    return EV2G_OK;
}

// a block of per-step rows: row i starts `stride` elements after row i - 1 (0: one row, overwritten); a null block has no rows
template <typename T>
struct Rows {
    T *p = nullptr;
    long long stride = 0;
    T *at(long long i) const { return p ? p + i * stride : nullptr; }
};

// The objects a handle owns (`list`: its heuristics, links, grids, wrappers, actor-critics or learners).  release_owned: where every one of
// them ends.  owned_check: the front of every *_check (`need_load` off for the kinds whose entries run without scenarios).  owned_created: the
// tail of every create behind its device stage's `rc`.  owned_destroy: nothing for an object the handle does not own, else out of the list,
// the stream drained, released.
template <typename T>
static void release_owned(T *x) {
    free_pool(x->allocs);
    free_pool(x->swap_allocs);
    delete x;
}
// (a learner leaves its policy first)
static void ppo_free(ev2g_ppo *p) {
    if (p->ac) p->ac->learner = nullptr;
    release_owned(p);
}
template <typename T>
static void release_all(std::vector<T *> &list, void (*release)(T *) = release_owned<T>) {
    for (T *x : list) release(x);
    list.clear();
}
template <typename T>
static int owned_check(ev2g_handle *h, std::vector<T *> ev2g_handle::*list, T *x, const char *thing, const char *who, bool need_load = true) {
    if (!h || !x) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (need_load && !h->loaded) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no scenarios loaded");
    if (std::find((h->*list).begin(), (h->*list).end(), x) == (h->*list).end())
        return fail(h, EV2G_ERR_ARG, std::string(who) + ": the " + thing + " was not created on this handle");
    (void)hipSetDevice(h->device);
    return EV2G_OK;
}
template <typename T>
static int owned_created(ev2g_handle *h, std::vector<T *> ev2g_handle::*list, T *x, int rc, T **out) {
    if (rc) {
        (void)hipStreamSynchronize(h->stream);   // (copies enqueued before the failure may still read host temporaries)
        release_owned(x);
        return rc;
    }
    (h->*list).push_back(x);
    *out = x;
    return EV2G_OK;
}
template <typename T>
static void owned_destroy(ev2g_handle *h, std::vector<T *> ev2g_handle::*list, T *x, void (*release)(T *) = release_owned<T>) {
    if (!h || !x) return;
    auto it = std::find((h->*list).begin(), (h->*list).end(), x);
    if (it == (h->*list).end()) return;
    (h->*list).erase(it);
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    release(x);
}

// a PortQueue of E envs x P ports into `pool`, empty (all zero); `powers`: with the two power lists
static int queue_alloc(ev2g_handle *h, std::vector<void *> &pool, int E, int P, bool powers, PortQueue *q) {
    const size_t EP = (size_t)E * P;
    if (int rc = dalloc(h, pool, EP, &q->queue)) return rc;
    if (int rc = dalloc(h, pool, (size_t)E, &q->qlen)) return rc;
    if (!powers) return EV2G_OK;
    if (int rc = dalloc(h, pool, EP, &q->qmin)) return rc;
    return dalloc(h, pool, EP, &q->qmax);
}

// ---- the step kernels' launch tables ----
// ev2g_route_host.h decides which instantiation a launch gets; these are the instantiations, one typed launch per entry, under the header's
// indices.  An entry that does not exist is null (and never instantiated): tuning builds with -DEV2G_ONLY_00 (tools/) keep the cfg2 plugin
// pair's and compile in seconds.
#ifdef EV2G_ONLY_00
constexpr bool kOnly00 = true;
#else
constexpr bool kOnly00 = false;
#endif
struct LaunchDims { dim3 grid; size_t lds; hipStream_t stream; };

typedef void (*WaveLaunch)(const LaunchDims &, const V2P *, const StepIO &, int t0, int k, int auto_reset, const WaveArgs &);
template <int SK, int RK, bool IO32, int FULLK>
static void launch_wave(const LaunchDims &d, const V2P *pp, const StepIO &io, int t0, int k, int auto_reset, const WaveArgs &wa) {
    hipLaunchKernelGGL((ev2g_step_wave<SK, RK, IO32, FULLK>), d.grid, dim3(EV2G_WAVE_BLOCK), d.lds, d.stream, pp, io, t0, k, auto_reset, wa, FusedArgs{});
}
template <int I>
constexpr WaveLaunch wave_entry() {   // I == route_wave_index(SK, RK, IO32, FULLK)
    constexpr int SK = I / 32, RK = I / 8 % 4, FULLK = I % 4;
    constexpr bool IO32 = I / 4 % 2 != 0;
    static_assert(route_wave_index(SK, RK, IO32, FULLK) == I, "the table's order is route_wave_index's");
    if constexpr (route_wave_exists(SK, RK, IO32, FULLK) && (!kOnly00 || (SK == 0 && RK == 0))) return &launch_wave<SK, RK, IO32, FULLK>;
    else return nullptr;
}

// ev2g_step_v2<block, SPEC>: the kernel (load_route sets its dynamic-LDS attribute) and its launch
struct V2Entry {
    const void *fn;
    void (*launch)(const LaunchDims &, const V2P *, const StepIO &, int t0, int k, int auto_reset);
};
template <int BLOCK, int SPEC>
static void launch_v2(const LaunchDims &d, const V2P *pp, const StepIO &io, int t0, int k, int auto_reset) {
    hipLaunchKernelGGL((ev2g_step_v2<BLOCK, SPEC>), d.grid, dim3(BLOCK), d.lds, d.stream, pp, io, t0, k, auto_reset);
}
template <int BLOCK, int SPEC>
static V2Entry v2_entry() { return {(const void *)ev2g_step_v2<BLOCK, SPEC>, &launch_v2<BLOCK, SPEC>}; }
static const V2Entry &v2_kernel(int block, bool spec) {
    static const V2Entry tab[3][2] = {{v2_entry<256, 0>(), v2_entry<256, 1>()}, {v2_entry<512, 0>(), v2_entry<512, 1>()}, {v2_entry<1024, 0>(), v2_entry<1024, 1>()}};
    return tab[block == 256 ? 0 : block == 512 ? 1 : 2][spec ? 1 : 0];
}

// the fused actor + step instantiations (FusedRoute::index): the kernel (launch_fused sets its dynamic-LDS attribute once per handle) and its launch
struct FusedEntry {
    const void *fn;
    void (*launch)(const LaunchDims &, const V2P *, const StepIO &, int t0, int k, const WaveArgs &, const FusedArgs &);
};
template <int SK, int RK, int AE, int NWF>
static void launch_fused_kernel(const LaunchDims &d, const V2P *pp, const StepIO &io, int t0, int k, const WaveArgs &wa, const FusedArgs &fa) {
    hipLaunchKernelGGL((ev2g_step_wave<SK, RK, true, 2, EV2G_FUSED_BLOCK, true, AE, NWF>), d.grid, dim3(EV2G_FUSED_BLOCK), d.lds, d.stream, pp, io, t0, k, 0, wa, fa);
}
template <int I>
static FusedEntry fused_entry() {
    constexpr FusedKey K = route_fused_key(I);
    static_assert(!K.exists || route_fused_index(K.sk, K.rk, K.ae, K.nwf) == I, "the table's order is route_fused_index's");
    if constexpr (K.exists && (!kOnly00 || K.sk == 0))
        return {(const void *)ev2g_step_wave<K.sk, K.rk, true, 2, EV2G_FUSED_BLOCK, true, K.ae, K.nwf>, &launch_fused_kernel<K.sk, K.rk, K.ae, K.nwf>};
    else return {nullptr, nullptr};
}

template <size_t... I>
constexpr std::array<WaveLaunch, sizeof...(I)> wave_table(std::index_sequence<I...>) { return {wave_entry<(int)I>()...}; }
template <size_t... I>
static std::array<FusedEntry, sizeof...(I)> fused_table(std::index_sequence<I...>) { return {fused_entry<(int)I>()...}; }
static constexpr std::array<WaveLaunch, ROUTE_WAVE_ENTRIES> kWaveTable = wave_table(std::make_index_sequence<ROUTE_WAVE_ENTRIES>{});
static const std::array<FusedEntry, ROUTE_FUSED_ENTRIES> kFusedTable = fused_table(std::make_index_sequence<ROUTE_FUSED_ENTRIES>{});

// ev2g_ac_act_kernel<activation>: the kernel (ev2g_ac_create sets its dynamic-LDS attribute) and its launch
struct AcEntry {
    const void *fn;
    void (*launch)(const LaunchDims &, const AcDev &, const float *x, int n_rows, int sample, uint64_t seed, uint64_t draw0, float *mean, float *actions,
                   float *clipped, float *value, float *log_prob);
};
template <int ACT>
static void launch_ac(const LaunchDims &d, const AcDev &dev, const float *x, int n_rows, int sample, uint64_t seed, uint64_t draw0, float *mean,
                      float *actions, float *clipped, float *value, float *log_prob) {
    hipLaunchKernelGGL(ev2g_ac_act_kernel<ACT>, d.grid, dim3(EV2G_AC_BLOCK), d.lds, d.stream, dev, x, n_rows, sample, seed, draw0, mean, actions, clipped,
                       value, log_prob);
}
template <int ACT>
static AcEntry ac_entry() { return {(const void *)ev2g_ac_act_kernel<ACT>, &launch_ac<ACT>}; }
static const AcEntry &ac_kernel(int relu) {
    static const AcEntry tab[2] = {ac_entry<EV2G_AC_TANH>(), ac_entry<EV2G_AC_RELU>()};
    return tab[relu ? 1 : 0];
}

// ev2g_ppo_grad_kernel<activation, head>: the kernel (ev2g_ppo_create sets its dynamic-LDS attribute) and its launch
struct PpoGradEntry {
    const void *fn;
    void (*launch)(const LaunchDims &, const AcDev &, const PpoDev &, const PpoLds &, const PpoHyper &, const float *obs, const float *actions,
                   const float *old_lp, const float *adv, const float *ret, const int *idx, int B, const double *advstat, float *work, double *stat_part);
};
template <int ACT, int HEAD>
static void launch_ppo_grad(const LaunchDims &d, const AcDev &ac, const PpoDev &dev, const PpoLds &lds, const PpoHyper &hp, const float *obs,
                            const float *actions, const float *old_lp, const float *adv, const float *ret, const int *idx, int B, const double *advstat,
                            float *work, double *stat_part) {
    hipLaunchKernelGGL((ev2g_ppo_grad_kernel<ACT, HEAD>), d.grid, dim3(EV2G_PPO_BLOCK), d.lds, d.stream, ac, dev, lds, hp, obs, actions, old_lp, adv, ret, idx, B, advstat,
                       work, stat_part);
}
template <int ACT, int HEAD>
static PpoGradEntry ppo_grad_entry() { return {(const void *)ev2g_ppo_grad_kernel<ACT, HEAD>, &launch_ppo_grad<ACT, HEAD>}; }
static const PpoGradEntry &ppo_grad_kernel(int relu, int head) {
    static const PpoGradEntry tab[2][2] = {{ppo_grad_entry<EV2G_AC_TANH, EV2G_HEAD_PPO>(), ppo_grad_entry<EV2G_AC_RELU, EV2G_HEAD_PPO>()},
                                           {ppo_grad_entry<EV2G_AC_TANH, EV2G_HEAD_A2C>(), ppo_grad_entry<EV2G_AC_RELU, EV2G_HEAD_A2C>()}};
    return tab[head ? 1 : 0][relu ? 1 : 0];
}

#include "ev2g_refill_host.h"

extern "C" {

int ev2g_abi_version(void) { return EV2G_ABI_VERSION; }

const char *ev2g_last_error(const ev2g_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ev2g_create(const ev2g_config *cfg, ev2g_handle **out) {
    if (!cfg || !out) return fail(nullptr, EV2G_ERR_ARG, "ev2g_create: null argument");
    if (cfg->reward_kind < 0 || cfg->reward_kind >= EV2G_N_REWARDS || cfg->state_kind < 0 || cfg->state_kind > 2)
        return fail(nullptr, EV2G_ERR_ARG, "ev2g_create: unknown reward_kind/state_kind");
    if (cfg->cost_kind == EV2G_COST_TR_OVERLOAD_USRPENALTY &&
        (cfg->reward_kind == EV2G_REWARD_SQTR_TRPENALTY_USERINCENTIVES || cfg->reward_kind >= EV2G_REWARD_V2G_PROFITMAX))
        return fail(nullptr, EV2G_ERR_ARG, "ev2g_create: the fused transformer_overload_usrpenalty cost shares its per-departure staging slot with "
                                           "the user term of this reward (SqTrError_TrPenalty_UserIncentives / V2G_profitmax / *V2G_profitmaxV2): evaluate one of the two on the host");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, EV2G_ERR_HIP, "ev2g_create: no HIP device visible (the engine has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= n) return fail(nullptr, EV2G_ERR_ARG, "ev2g_create: device ordinal out of range");
    ev2g_handle *h = new ev2g_handle();
    h->cfg = *cfg;
    h->device = cfg->device;
    if (hipSetDevice(h->device) != hipSuccess) {
        delete h;
        return fail(nullptr, EV2G_ERR_HIP, "ev2g_create: hipSetDevice failed");
    }
    if (cfg->stream) {
        h->stream = (hipStream_t)cfg->stream;
    } else if (cfg->flags & EV2G_FLAG_NULL_STREAM) {
        h->stream = nullptr;  // legacy default stream
    } else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
            delete h;
            return fail(nullptr, EV2G_ERR_HIP, "ev2g_create: hipStreamCreate failed");
        }
        h->own_stream = true;
    }
    for (int i = 0; i < EV2G_EV_RING; i++) { (void)hipEventCreate(&h->ev0s[i]); (void)hipEventCreate(&h->ev1s[i]); }
    // the stamp pairs and the rate of the clock they hold (a device that reports none keeps the event pairs: stamps_usable)
    if (hipDeviceGetAttribute(&h->wall_khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess) h->wall_khz = 0;
    if (int rc = dalloc(h, h->life_allocs, (size_t)EV2G_EV_RING * 2, &h->d_stamps)) {
        g_create_error = "ev2g_create: " + h->err;
        ev2g_destroy(h);
        return rc;
    }
    *out = h;
    return EV2G_OK;
}

// captured rollout segments hold kernel arguments (device pointers, shapes, actor weights) of the moment they were recorded
static void drop_rollout_graphs(ev2g_handle *h) {
    for (auto &g : h->rollout_graphs) (void)hipGraphExecDestroy(g.exec);
    h->rollout_graphs.clear();
}

void ev2g_destroy(ev2g_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    free_pool(h->scn_allocs);
    free_pool(h->st_allocs);
    free_pool(h->user_allocs);
    free_pool(h->life_allocs);
    for (void *p : h->user_host_allocs) (void)hipHostFree(p);
    h->user_host_allocs.clear();
    if (h->peek_stage) (void)hipHostFree(h->peek_stage);
    free_pool(h->refill_cache.allocs);
    if (h->d_refill_overflow) (void)hipFree(h->d_refill_overflow);
    release_all(h->heuristics);
    release_all(h->links);
    release_all(h->grids);
    release_all(h->wraps);
    release_all(h->ppos, ppo_free);   // (learners before their policies)
    release_all(h->td3s, td3_free);
    release_all(h->sacs);
    release_all(h->tqcs);
    release_all(h->arss);
    release_all(h->acs);
    ev2g_comm_destroy(h);
    drop_rollout_graphs(h);
    for (int i = 0; i < EV2G_EV_RING; i++) { if (h->ev0s[i]) (void)hipEventDestroy(h->ev0s[i]); if (h->ev1s[i]) (void)hipEventDestroy(h->ev1s[i]); }
    if (h->own_stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int ev2g_n_envs(const ev2g_handle *h) { return h ? h->E : 0; }
int ev2g_n_ports(const ev2g_handle *h) { return h ? h->P : 0; }
int ev2g_obs_dim(const ev2g_handle *h) { return h ? h->D : 0; }
int ev2g_n_steps(const ev2g_handle *h) { return h ? h->T : 0; }
int ev2g_current_step(const ev2g_handle *h) { return h ? h->current_step : 0; }
const char *ev2g_kernel_name(const ev2g_handle *h) { return (h && h->loaded) ? h->kernel_name.c_str() : ""; }
const char *ev2g_fallback_reason(const ev2g_handle *h) { return (h && h->loaded) ? h->fallback_reason.c_str() : ""; }
const char *ev2g_big_kernel_reason(const ev2g_handle *h) { return (h && h->loaded) ? h->big_reason.c_str() : ""; }
int ev2g_last_launch_specialisation(const ev2g_handle *h) { return (h && h->loaded) ? h->last.specialisation : -1; }
int ev2g_last_stats_route(const ev2g_handle *h) { return (h && h->loaded) ? h->last_stats_route : -1; }
const char *ev2g_last_stats_reason(const ev2g_handle *h) { return (h && h->loaded && h->last_stats_route == 0) ? h->stats_reason : ""; }
int ev2g_last_launch_fast_forwarded(ev2g_handle *h, int64_t *steps, int64_t *stretches) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_last_launch_fast_forwarded: no scenarios loaded");
    int64_t n = 0, m = 0;
    if (h->last.ff) {   // the counts of the launch's workgroups, summed on demand
        (void)hipSetDevice(h->device);
        std::vector<unsigned long long> c((size_t)h->scn.n_groups);
        HIPCHK(h, hipMemcpyAsync(c.data(), h->d_ff_count, sizeof(unsigned long long) * c.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (unsigned long long v : c) { n += (int64_t)(v & 0xffffffffull); m += (int64_t)(v >> 32); }
    }
    if (steps) *steps = n;
    if (stretches) *stretches = m;
    return EV2G_OK;
}
int ev2g_last_launch_balance(const ev2g_handle *h, int64_t *moved, const char **reason) {
    const bool on = h && h->loaded && h->last.balance;
    if (moved) *moved = on ? h->last_balance_moved : 0;
    if (reason) *reason = (h && h->loaded) ? (on ? "" : h->last.balance_reason) : "no scenarios loaded";
    return on ? 1 : 0;
}
int ev2g_last_launch_placement(ev2g_handle *h, uint32_t *out, int64_t n_words) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_last_launch_placement: no scenarios loaded");
    if (!h->d_place || !h->last.ff) return 0;   // (not loaded with EV2G_PLACEMENT=1, or the last launch does not fast-forward: nothing was recorded)
    const int64_t n = 2 * (int64_t)h->scn.n_groups;
    if (!out || n_words < n) return fail(h, EV2G_ERR_ARG, "ev2g_last_launch_placement: out must hold two words per workgroup");
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipMemcpyAsync(out, h->d_place, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return (int)h->scn.n_groups;
}
const char *ev2g_last_launch_general_reason(const ev2g_handle *h) { return (h && h->loaded && h->last.specialisation == 0) ? h->last.general_reason : ""; }

static const char *kStatNames[EV2G_N_STATS] = {
    "total_ev_served", "total_profits", "total_energy_charged", "total_energy_discharged",
    "average_user_satisfaction", "power_tracker_violation", "tracking_error", "energy_tracking_error",
    "energy_user_satisfaction", "std_energy_user_satisfaction", "min_energy_user_satisfaction",
    "total_steps_min_emergency_battery_capacity_violation", "total_transformer_overload",
    "battery_degradation", "battery_degradation_calendar", "battery_degradation_cycling", "total_reward"};
const char *ev2g_stat_name(int i) { return (i >= 0 && i < EV2G_N_STATS) ? kStatNames[i] : ""; }

int ev2g_reset_ex(ev2g_handle *h, double *obs, int64_t scenario_offset);

// Envs per wavefront of ev2g_stats_kernel (the summation order of its reductions follows from it): two where an env's sessions fit 32 lanes with
// room to spare (PublicPST: ~14 per env -- 74.6 -> 58.0 us at cfg3; at cfg2's ~35 per env half of the lanes would need a second pass: 47 -> 52 us,
// so it keeps a wavefront per env).  Refillable pools: by the session slots per scenario, not by what the loaded batch happened to hold -- the
// choice (and the summation order) stays put across refills.
static bool stats_pair(const ev2g_handle *h) {
    const long long per_scn = h->sess_cap > 0 ? (long long)h->sess_cap : (h->S + h->M - 1) / std::max(h->M, 1);
    return (h->sess_cap > 0 ? per_scn <= 48 : h->S <= (long long)h->M * 24) && h->C <= 32;
}

// ---- ev2g_load_scenarios: the device stage ----
// ev2g_load_host.h plans on the host (layout, session order, constants, records, dictionary); the load_* functions below route the plan to
// a kernel, upload it, build the device tables and allocate the state, in the order ev2g_load_scenarios calls them.

// Kernel routing and launch geometry.  Fast path (ev2g_step_wave): the common shape.  Anything else runs the general kernels; which one was
// chosen, and why the fast path was not, is reported by ev2g_kernel_name() / ev2g_fallback_reason() -- routing is never silent.
static int load_route(ev2g_handle *h, const LoadPlan &p, const LoadSwitches &sw) {
    const int E = p.E, M = p.M, T = p.T, C = p.C, npc = p.npc, P = p.P, R = p.R, D = p.D, sk = h->cfg.state_kind;
    DevScn &s = h->scn;
    s = DevScn{};
    s.E = E; s.M = M; s.T = T; s.C = C; s.npc = npc; s.P = P; s.R = R; s.D = D; s.ND = std::max(p.ND, 1); s.dt = p.dt;
    s.reward_kind = h->cfg.reward_kind; s.state_kind = sk; s.flags = h->cfg.flags; s.cost_kind = h->cfg.cost_kind; s.n_lut = p.n_lut;
    s.het = p.het ? 1 : 0;
    RouteShape &rs = h->shape;
    rs = RouteShape{};
    rs.P = P; rs.T = T; rs.D = D; rs.npc = npc; rs.state_kind = sk; rs.reward_kind = h->cfg.reward_kind; rs.flags = h->cfg.flags;
    // v2 kernel: one home lane per port, BLOCK >= P; the generic kernel handles larger envs
    rs.block = p.het ? 0 : (P <= 256) ? 256 : (P <= 512) ? 512 : (P <= 1024) ? 1024 : 0;   // different port counts per charger: generic kernel
    const int blk = rs.block ? rs.block : EV2G_BLOCK;
    s.G = std::max(1, blk / P);
    s.G = std::min(s.G, E);
    h->fallback_reason.clear();
    if (P < 2 || P > 64) h->fallback_reason = "ports per env outside 2..64";
    else if (R != 1) h->fallback_reason = "more than one transformer";
    else if (npc != 1) h->fallback_reason = "multi-port chargers";
    if (p.het) h->fallback_reason = "chargers with different port counts (topology file)";
    bool wave = h->fallback_reason.empty();
    rs.no_full = sw.no_full; rs.no_wide = sw.no_wide; rs.no_strided = sw.no_strided; rs.no_inl_stats = sw.no_inl_stats;
    h->last = StepRoute{}; h->last.inl_reason = "no step launch since the scenarios were loaded"; h->last_stats_route = -1;
    h->state_epoch += 1;
    if (wave) {   // ev2g_step_wave addresses every array as base + 32-bit byte offset: all of them must stay below 4 GiB
        const unsigned long long lim = 1ull << 32;
        const unsigned long long biggest = std::max({(unsigned long long)E * P * 8, (unsigned long long)E * D * 8,
                                                     (unsigned long long)M * (T + 1) * 60 * 8, (unsigned long long)p.SD * sizeof(SessRec),
                                                     (unsigned long long)M * T * 64, (unsigned long long)E * T * 8 * 3, (unsigned long long)M * P * 8, (unsigned long long)E * P * sizeof(PortLine),
                                                     (h->cfg.flags & EV2G_FLAG_LOG_SOC) ? (unsigned long long)E * T * P * 8 : 0ull,
                                                     (h->cfg.flags & EV2G_FLAG_LOG_CS_HISTORY) ? (unsigned long long)T * E * C * 8 : 0ull});
        if (biggest >= lim) { wave = false; h->fallback_reason = "an array of the batch reaches 4 GiB (32-bit byte offsets)"; }
    }
    if (wave && sw.kernel_v2) {   // EV2G_KERNEL=v2 forces the general kernel on the common shape (parity tests compare the two)
        wave = false; h->fallback_reason = "EV2G_KERNEL=v2";
    }
    rs.family = wave ? ROUTE_WAVE : rs.block ? ROUTE_V2 : ROUTE_GENERIC;   // (load_route_big: ROUTE_V2 -> ROUTE_BIG)
    if (wave) {   // wave-aligned: 64/P envs per wavefront, packed
        rs.epw = 64 / P;
        s.G = (EV2G_WAVE_BLOCK / 64) * rs.epw;
        if (p.n_lut > 4094) rs.no_full = true;   // the full kernels keep table id + 1 in 12 bits of a port's LDS word
    }
    {
        char nm[64];
        if (wave) std::snprintf(nm, sizeof nm, "ev2g_step_wave<%d,%d>", sk, std::min(h->cfg.reward_kind, 3));
        else if (rs.block) std::snprintf(nm, sizeof nm, "ev2g_step_v2<%d>", rs.block);
        else std::snprintf(nm, sizeof nm, "ev2g_step_kernel");
        h->kernel_name = nm;
    }
    {
        int gs = 4;
        while (gs < 64 && gs < p.max_seg) gs <<= 1;
        s.gs = gs;
    }
    s.n_groups = (E + s.G - 1) / s.G;
    s.sixty_over_dt = 60.0 / (double)p.dt;
    s.dt_over_60 = (double)p.dt / 60.0;
    if (wave)
        h->lds_bytes = ev2g_wave_lds_bytes(s.G);
    else if (rs.block)
        h->lds_bytes = ev2g_v2_lds_bytes(s.G * P, s.G * R, s.G, R);
    else
        h->lds_bytes = ev2g_generic_lds_bytes(s.G, P, R, npc);
    if (h->lds_bytes > 160 * 1024)
        return fail(h, EV2G_ERR_ARG, "ev2g_load_scenarios: ports per env exceed the LDS staging capacity (P <= ~2400)");
    if (h->lds_bytes > 48 * 1024) {
        HIPCHK(h, hipFuncSetAttribute(rs.block ? v2_kernel(rs.block, false).fn : (const void *)ev2g_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
        if (rs.block) HIPCHK(h, hipFuncSetAttribute(v2_kernel(rs.block, true).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
    }
    return EV2G_OK;
}

// ev2g_step_big (ev2g_step_big.h): big single-env workgroups with two ports per home lane.  What it needs beyond the launch-time conditions
// of the specialised instantiation: single-port chargers, at most 50 transformers, at most EV2G_BIG_NCC distinct charger tuples, windows that fit
// 16-bit step numbers.  EV2G_NO_BIG keeps ev2g_step_v2<1024> (A/B runs, parity tests).
static int load_route_big(ev2g_handle *h, LoadPlan &p, const ev2g_scenario_batch *b, const LoadSwitches &sw) {
    h->big_reason.clear(); h->big_args = BigArgs{};
    if (h->shape.block != 1024 || h->shape.wave()) return EV2G_OK;
    load_plan_big(p, b, EV2G_BIG_NCC);
    const size_t lb = ev2g_big_lds_bytes(p.P, p.R);
    if (sw.no_big) h->big_reason = "EV2G_NO_BIG is set";
    else if (p.npc != 1) h->big_reason = "multi-port chargers";
    else if (h->cfg.state_kind != EV2G_STATE_V2G_PROFIT_MAX_LOADS) h->big_reason = "the state function is not V2G_profit_max_loads";
    else if (20 * p.R + 20 > 2 * EV2G_BIG_BLOCK) h->big_reason = "more than 50 transformers (their 20 R window-column pairs + 20 price columns ride in 1024 pair slots)";
    else if (p.many) h->big_reason = "more than 16 distinct charger constant tuples";
    else if (p.tmax > EV2G_BIG_TMAX / 2 || p.tmin < -1) h->big_reason = "a session window or the episode length exceeds 16383 steps";
    else if (!p.even || p.D >= 65536) h->big_reason = "observation columns are not 16-byte aligned pairs";
    else if (lb > 80 * 1024) h->big_reason = "the port state exceeds half of a CU's LDS";
    else if (p.E < 1) h->big_reason = "no envs";
    else {
        h->big_args.ncc = (int)(p.ctab.size() / 6);
        h->lds_big = lb; h->shape.family = ROUTE_BIG;
        HIPCHK(h, hipFuncSetAttribute((const void *)ev2g_step_big<EV2G_BIG_BLOCK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb));
    }
    return EV2G_OK;
}

// Copies the plan and the batch's own arrays to the device (asynchronously: the plan outlives the stream synchronisation that ends the load).
// *d_lut_eta: the efficiency tables as efficiencies, what V2P::lut points at.
static int load_upload(ev2g_handle *h, const LoadPlan &p, const ev2g_scenario_batch *b, double **d_lut_eta) {
    DevScn &s = h->scn;
    auto &pool = h->scn_allocs;
    const int M = p.M, T = p.T, C = p.C, R = p.R;
    int rc = 0;
#define UP(dst, vec) if ((rc = upload(h, pool, (vec).data(), (vec).size(), &(dst)))) return rc;
#define UPP(dst, ptr, n) if ((rc = upload(h, pool, (ptr), (size_t)(n), &(dst)))) return rc;
    int *ip; double *dp;
    UP(ip, p.slot_port) s.slot_port = ip;
    UP(ip, p.slot_cs) s.slot_cs = ip;
    UP(ip, p.slot_obs) s.slot_obs = ip;
    UP(ip, p.slot_tr) s.slot_tr = ip;
    UP(ip, p.slot_mask) s.slot_mask = ip;
    UP(ip, p.np_of) s.cs_np = ip;
    UP(ip, p.pbase) s.cs_pbase = ip;
    UP(ip, p.cs_slot0) s.cs_slot0 = ip;
    UPP(dp, b->cs_min_charge_current, C) s.cs_imin = dp;
    UPP(dp, b->cs_max_charge_current, C) s.cs_imax = dp;
    UPP(dp, b->cs_min_discharge_current, C) s.cs_dmin = dp;
    UP(dp, p.cs_dmax_abs) s.cs_dmax_abs = dp;
    UPP(dp, b->cs_voltage, C) s.cs_volt = dp;
    UP(dp, p.cs_maxp) s.cs_maxp = dp;
    UP(dp, p.cs_minp) s.cs_minp = dp;
    UP(dp, p.cs_vk) s.cs_vk = dp;
    h->heur_avg_power = p.avg_power; h->heur_min_action = p.min_action;
    UP(dp, p.cs_kw) h->d_heur_cs_kw = dp;
    UP(dp, p.cs_min_kw) h->d_heur_cs_min_kw = dp;
    UP(ip, p.port_slot) h->d_port_slot = ip;
    UP(dp, p.cs_pack) s.cs_pack = dp;
    if (h->shape.big()) {
        unsigned char *cp; UP(cp, p.ccls) h->big_args.slot_ccls = cp;
        UP(dp, p.ctab) h->big_args.ccls_tab = dp;
        UP(dp, p.ptab) h->big_args.potc_tab = dp;
    }
    UPP(ip, b->cs_phases, C) s.cs_ph = ip;
    UP(ip, p.tr_seg) s.tr_seg = ip;
    UP(ip, p.tr_obs) s.tr_obs = ip;
    UPP(dp, b->charge_price, (size_t)M * T) s.price_ch = dp;
    UPP(dp, b->discharge_price, (size_t)M * T) s.price_dis = dp;
    UPP(dp, b->power_setpoints, (size_t)M * T) s.setpoint = dp;
    UPP(dp, b->tr_max_power, (size_t)M * R * T) s.tr_maxp = dp;
    UPP(dp, b->tr_min_power, (size_t)M * R * T) s.tr_minp = dp;
    UPP(dp, b->tr_inflexible_load, (size_t)M * R * T) s.tr_infl = dp;
    UPP(dp, b->tr_solar_power, (size_t)M * R * T) s.tr_solar = dp;
    UPP(dp, b->tr_load_forecast, (size_t)M * R * T) s.tr_lf = dp;
    UPP(dp, b->tr_pv_forecast, (size_t)M * R * T) s.tr_pvf = dp;
    UP(dp, p.tr_peak) s.tr_peak = dp;
    UP(dp, p.tr_base) s.tr_base = dp;
    UPP(dp, b->tr_dr, (size_t)M * R * p.ND * 3) s.tr_dr = dp;
    UPP(ip, b->tr_n_dr, (size_t)M * R) s.tr_ndr = ip;
    UPP(ip, b->tr_steps_ahead, (size_t)M * R) s.tr_ahead = ip;
    UP(ip, p.ss_tarr) s.ss_tarr = ip;
    UP(ip, p.ss_tdep) s.ss_tdep = ip;
    UP(ip, p.ss_ntarr) s.ss_ntarr = ip;
    UP(ip, p.ss_ntdep) s.ss_ntdep = ip;
    UP(ip, p.ss_phases) s.ss_phases = ip;
    UP(ip, p.ss_lut) s.ss_lut = ip;
    UP(dp, p.ss_cap0) s.ss_cap0 = dp;
    UP(dp, p.ss_B) s.ss_B = dp;
    UP(dp, p.ss_des) s.ss_des = dp;
    UP(dp, p.ss_minB) s.ss_minB = dp;
    UP(dp, p.ss_emerg) s.ss_emerg = dp;
    UP(dp, p.ss_pacmax) s.ss_pacmax = dp;
    UP(dp, p.ss_pacmin) s.ss_pacmin = dp;
    UP(dp, p.ss_pdismax) s.ss_pdismax = dp;
    UP(dp, p.ss_pdismin) s.ss_pdismin = dp;
    UP(dp, p.ss_ts) s.ss_ts = dp;
    UP(dp, p.ss_tsm) s.ss_tsm = dp;
    UP(dp, p.ss_etach) s.ss_etach = dp;
    UP(dp, p.ss_etadis) s.ss_etadis = dp;
    UPP(dp, b->lut, (size_t)p.n_lut * EV2G_LUT_LEN) s.lut = dp;
    UP(*d_lut_eta, p.lut_eta)
    UP(dp, p.rowmax) h->d_lut_rowmax = dp;
    UP(ip, p.port_first) s.port_first = ip;
    UP(ip, p.port_end) s.port_end = ip;
    UP(ip, p.ss_slot) s.ss_slot = ip;
    UP(ip, p.scn_sess) s.scn_sess = ip;
    UP(ip, p.scn_sess_end) s.scn_sess_end = ip;
    static_assert(sizeof(IntPair) == sizeof(int2), "port_first_win is uploaded as int2");
    { int2 *i2p; UPP(i2p, (const int2 *)p.port_first_win.data(), p.port_first_win.size()) s.port_first_win = i2p; }
    UP(dp, p.ss_afap) h->d_ss_afap = dp;
    { SessRec *rp; UP(rp, p.recs) s.rec = rp; }
    { SessTail *tp; UP(tp, p.tails) s.tail = tp; }
    s.sess_dyn = nullptr; s.cls_rec = nullptr; s.dict = 0; s.n_cls = 0; h->d_cls_rec = nullptr;
    if (h->shape.wave()) {
        SessDyn *dp2; UP(dp2, p.dyns) s.sess_dyn = dp2;
        ClsRec *cp; UP(cp, p.cls_tab) s.cls_rec = cp; h->d_cls_rec = cp;
        s.dict = p.dict ? 1 : 0; s.n_cls = p.dict ? (int)p.cls_map.size() : 0;
    }
#undef UP
#undef UPP
    return EV2G_OK;
}

// The tables the device builds from the uploaded scenarios: the forecast / limit windows of the V2G_profit_max_loads state, and the
// fast path's step table (with its occupancy masks) and observation head table.
static int load_build_tables(ev2g_handle *h) {
    DevScn &s = h->scn;
    auto &pool = h->scn_allocs;
    const int M = s.M, T = s.T, R = s.R, sk = s.state_kind;
    s.win_tab = nullptr;
    if (sk == EV2G_STATE_V2G_PROFIT_MAX_LOADS && h->shape.block) {
        double *tab = nullptr;
        const size_t n = (size_t)M * R * (T + 1) * 40;
        HIPCHK(h, hipMalloc((void **)&tab, n * sizeof(double)));
        pool.push_back(tab);
        const int nb = (int)std::min<size_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(ev2g_build_window_table_kernel, dim3(nb), dim3(256), 0, h->stream, s, tab, 0, M);
        HIPCHK(h, hipGetLastError());
        s.win_tab = tab;
    }
    h->d_step_tab = nullptr;
    if (h->shape.wave()) {   // R == 1: [M,T] series interleaved per (env, step)
        double *d_step_tab = nullptr;
        const size_t n = (size_t)M * T * 8;
        HIPCHK(h, hipMalloc((void **)&d_step_tab, n * sizeof(double)));
        pool.push_back(d_step_tab);
        const int nb = (int)std::min<size_t>(((size_t)M * T + 255) / 256, 4096);
        hipLaunchKernelGGL(ev2g_build_step_table_kernel, dim3(nb), dim3(256), 0, h->stream, s, d_step_tab, 0, M);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(ev2g_build_occ_mask_kernel, dim3(std::min(M, 8192)), dim3(64), 0, h->stream, s, d_step_tab, 0, M);   // slots 6, 7
        HIPCHK(h, hipGetLastError());
        h->d_step_tab = d_step_tab;
    }
    h->d_head_tab = nullptr; h->head_nh = 0;
    s.head_tab = nullptr; s.head_nh = 0;
    if (h->shape.wave() && sk != EV2G_STATE_PUBLIC_PST) {
        double *d_head_tab = nullptr;
        const int NH = (sk == EV2G_STATE_V2G_PROFIT_MAX_LOADS) ? 60 : 20;
        const size_t n = (size_t)M * (T + 1) * NH;
        HIPCHK(h, hipMalloc((void **)&d_head_tab, n * sizeof(double)));
        pool.push_back(d_head_tab);
        const int nb = (int)std::min<size_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(ev2g_build_head_table_kernel, dim3(nb), dim3(256), 0, h->stream, s.price_ch, s.win_tab, 0, M, T, NH, d_head_tab);
        HIPCHK(h, hipGetLastError());
        h->d_head_tab = d_head_tab; h->head_nh = NH;
        s.head_tab = d_head_tab; s.head_nh = NH;   // (the reset observation copies its head from row 0, write_obs_env)
    }
    return EV2G_OK;
}

// The envs' state (zeroed), for `SD` device session slots
static int load_alloc_state(ev2g_handle *h, long long SD) {
    const DevScn &s = h->scn;
    DevState &st = h->st;
    st = DevState{};
    auto &sp = h->st_allocs;
    const int E = s.E, T = s.T, R = s.R;
    const size_t EP = (size_t)E * s.P, EC = (size_t)E * s.C;
    int rc = 0;
#define AL(field, n) if ((rc = dalloc(h, sp, (size_t)(n), &st.field))) return rc;
    {   // per-port state: one 64-byte line per port + one slab of EV2G_PS_* slices for what is not on the step's path
        AL(line, EP)
        HIPCHK(h, hipMemsetAsync(st.line, 0, EP * sizeof(PortLine), h->stream));
        if (h->shape.wave()) { AL(port_dyn, EP) }
        const size_t slice = std::max(EP, EC) * 8;
        if ((rc = dalloc(h, sp, slice * EV2G_PS_N, &st.slab_port))) return rc;
        st.slab_port_slice = slice;
#define SLICE(T, k) ((T *)(st.slab_port + slice * (size_t)(k)))
        st.port_energy = SLICE(double, EV2G_PS_PENERGY); st.port_current = SLICE(double, EV2G_PS_PCURRENT);
        st.cs_sat_sum = SLICE(double, EV2G_PS_SATSUM); st.cs_served = SLICE(int, EV2G_PS_SERVED);
#undef SLICE
    }
    if (h->cfg.flags & EV2G_FLAG_LOG_CS_HISTORY) {
        AL(cs_profits, EC) AL(cs_e_ch, EC) AL(cs_e_dis, EC) AL(cs_power_now, EC) AL(cs_cur_now, EC)
        AL(cs_power_hist, (size_t)T * EC) AL(cs_cur_hist, (size_t)T * EC)
    }
    AL(env_acc, (size_t)E * 8) AL(env_fault, E)
    AL(slab_hist, (size_t)T * E * (2 + R))
    st.hist = st.slab_hist;
    AL(slab_sess, (size_t)std::max<long long>(SD, 1) * 2)
    st.sess_final_cap = st.slab_sess;
    AL(tr_power_now, (size_t)E * R)
    if (h->cfg.flags & EV2G_FLAG_LOG_SOC) { AL(soc_log, (size_t)T * EP) st.sess_abs_e = st.slab_sess + (size_t)std::max<long long>(SD, 1); }
#ifdef EV2G_PHASE_TIMING
    AL(dbg, (size_t)s.n_groups * 18)
#endif
#undef AL
    return EV2G_OK;
}

// The device copy of the v2 kernels' parameter block.  `v2p` is the caller's: the copy is asynchronous, so the block lives where the
// stream synchronisation that ends the load is.
static int load_params(ev2g_handle *h, double *d_lut_eta, V2P &v2p) {
    ev2g_v2_fill_params(v2p, h->scn, h->st);
    EV2G_SETP(v2p.lut, d_lut_eta);
    EV2G_SETP(v2p.head_tab, h->d_head_tab);
    EV2G_SETP(v2p.step_tab, h->d_step_tab);
    EV2G_SETP(v2p.ss_afap, h->d_ss_afap);
    int ex = 0;   // 60/dt a power of two and dt/60 its exact reciprocal -> divisions by them are multiplications
    v2p.pow2_dt = (std::frexp(h->scn.sixty_over_dt, &ex) == 0.5 && h->scn.sixty_over_dt * h->scn.dt_over_60 == 1.0) ? 1 : 0;
    h->shape.pow2_dt = v2p.pow2_dt != 0;
    return upload(h, h->st_allocs, &v2p, 1, &h->d_v2p);
}

// The in-launch statistics phase: a shape the statistics kernel runs with one env per wavefront (its summation order), like the phase
static int load_decide_inl_stats(ev2g_handle *h, const LoadSwitches &sw) {
    RouteShape &rs = h->shape;
    h->d_stats_inl = nullptr;
    const char *why = "";
    if (rs.no_inl_stats) why = "EV2G_NO_INLAUNCH_STATS is set";
    else if (!rs.wave() || !(h->cfg.flags & EV2G_FLAG_LOG_SOC)) why = "the step kernel is not ev2g_step_wave with the SoC log";
    else if (rs.epw != 1 || stats_pair(h)) why = "several envs per wavefront (the in-launch phase computes one env per wavefront, like the statistics kernel at this shape)";
    else if (h->lds_bytes < ev2g_inl_stats_lds_bytes()) why = "the step kernel's LDS is smaller than the phase's blocks";
    rs.inl_shape_reason = why;
    h->d_ff_count = nullptr; h->d_place = nullptr;
    if (rs.wave() && rs.epw == 1 && !sw.no_fast_forward) {   // the fast-forward's per-workgroup counts: what switches it on
        int rc = 0;
        if ((rc = dalloc(h, h->st_allocs, (size_t)h->scn.n_groups, &h->d_ff_count))) return rc;
        unsigned long long *p = h->d_ff_count;
        HIPCHK(h, hipMemcpy((char *)h->d_v2p + offsetof(V2P, ff_count), &p, sizeof p, hipMemcpyHostToDevice));
        if (sw.placement) {   // (development) the same launches record where their workgroups ran
            if ((rc = dalloc(h, h->st_allocs, 2 * (size_t)h->scn.n_groups + 2048, &h->d_place))) return rc;
            unsigned *q = h->d_place;
            HIPCHK(h, hipMemcpy((char *)h->d_v2p + offsetof(V2P, place), &q, sizeof q, hipMemcpyHostToDevice));
        }
    }
    if (!why[0]) {
        int rc = 0;
        if ((rc = dalloc(h, h->st_allocs, (size_t)h->E * EV2G_N_STATS, &h->d_stats_inl))) return rc;
        double *p = h->d_stats_inl;
        HIPCHK(h, hipMemcpy((char *)h->d_v2p + offsetof(V2P, stats_inl), &p, sizeof p, hipMemcpyHostToDevice));
    }
    rs.ff_count = h->d_ff_count != nullptr; rs.stats_inl = h->d_stats_inl != nullptr;
    return EV2G_OK;
}

// CU balance (ev2g_balance_host.h).  The map of the pool window at `off`, on the device: kept from the launch that first started there (or from the
// load, which builds those of the windows an episode loop over the pool visits: offsets k * E), in one of kBalanceSlots slots that are reused oldest
// first -- the copy into a slot is ordered on the handle's stream behind the launches that read it.  nullptr: the copy failed, the kernel's own map holds.
constexpr size_t kBalanceSlots = 64;
static const int *balance_get(ev2g_handle *h, long long off) {
    const size_t n = (size_t)h->scn.n_groups;
    for (size_t i = 0; i < h->balance_maps.size(); i++)
        if (h->balance_maps[i].off == off) { h->last_balance_moved = h->balance_maps[i].moved; return h->d_balance + i * n; }
    const size_t slot = h->balance_next;
    h->balance_next = (slot + 1) % kBalanceSlots;
    if (h->balance_maps.size() <= slot) h->balance_maps.emplace_back();
    ev2g_handle::BalanceMap &m = h->balance_maps[slot];
    std::vector<int> weight;
    balance_group_weights(h->balance_bits, h->M, off, h->E, 4, weight);
    m.moved = balance_map(weight, h->balance_cus, m.host);
    m.off = off;
    if (m.host.size() != n || hipMemcpyAsync(h->d_balance + slot * n, m.host.data(), n * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess) {
        m.off = -1;
        return nullptr;
    }
    h->last_balance_moved = m.moved;
    return h->d_balance + slot * n;
}

// Which launches may be balanced (RouteShape::balance; route_step adds the launch's own conditions), and what the maps are made from
static int load_balance(ev2g_handle *h, const ev2g_scenario_batch *b, const LoadSwitches &sw) {
    RouteShape &rs = h->shape;
    h->balance_bits.clear(); h->balance_maps.clear();
    h->d_balance = nullptr; h->balance_next = 0; h->last_balance_moved = 0;
    const char *why = "";
    if (sw.no_cu_balance) why = "EV2G_NO_CU_BALANCE is set";
    else if (!rs.ff_count) why = "the loaded shape never fast-forwards (another kernel, several envs per wavefront, or EV2G_NO_FAST_FORWARD)";
    else if (h->T > BALANCE_MAX_T) why = "an episode has more than 256 steps";
    else if (h->cfg.flags & EV2G_FLAG_REFILLABLE) why = "the handle is EV2G_FLAG_REFILLABLE (a refill changes the scenarios the maps were made from)";
    else if (h->scn.n_groups != (h->E + 3) / 4) why = "a workgroup does not step four envs";
    rs.balance_shape_reason = why;
    rs.balance = why[0] == 0;
    if (!rs.balance) return EV2G_OK;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus < 8) cus = 256;
    h->balance_cus = cus;
    h->balance_bits.resize((size_t)h->M * BALANCE_WORDS);
    for (long long m = 0; m < h->M; m++) {
        const int64_t s0 = b->env_session_start[m], s1 = b->env_session_start[m + 1];
        balance_live_bits(b->ev_t_arr + s0, b->ev_t_dep + s0, s1 - s0, h->T, &h->balance_bits[(size_t)m * BALANCE_WORDS]);
    }
    int rc = 0;
    if ((rc = dalloc(h, h->st_allocs, kBalanceSlots * (size_t)h->scn.n_groups, &h->d_balance))) return rc;
    for (long long k = 0; k < std::min<long long>(h->M / h->E, (long long)kBalanceSlots); k++)
        if (!balance_get(h, k * h->E)) return fail(h, EV2G_ERR_HIP, "ev2g_load_scenarios: a CU-balance map could not be uploaded");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->last_balance_moved = 0;
    return EV2G_OK;
}

int ev2g_load_scenarios(ev2g_handle *h, const ev2g_scenario_batch *b) {
    if (!h || !b) return fail(h, EV2G_ERR_ARG, "ev2g_load_scenarios: null argument");
    (void)hipSetDevice(h->device);
    const LoadSwitches sw = load_switches_from_env();
    LoadPlan plan;   // the uploads copy out of its vectors, and out of v2p, asynchronously: every return below load_upload synchronises the stream first
    V2P v2p;
    std::string msg;
    int rc = load_plan_check(plan, b, h->cfg, msg);
    if (rc) return fail(h, rc, msg);   // (a pool loaded earlier stays loaded and usable; from here on a refusal leaves the handle unloaded)
    (void)hipStreamSynchronize(h->stream);
    drop_rollout_graphs(h);
    free_pool(h->scn_allocs);
    free_pool(h->st_allocs);
    h->loaded = false;
    h->timing_events = sw.timing_events;
    h->cls_map.clear();

    if ((rc = load_plan_layout(plan, b, h->cfg, sw, msg))) return fail(h, rc, msg);
    h->sess_cap = (int)plan.cap;
    if ((rc = load_plan_order(plan, b, msg))) return fail(h, rc, msg);
    load_plan_constants(plan, b);
    load_plan_records(plan, b);
    if ((rc = load_route(h, plan, sw))) return rc;
    load_plan_dictionary(plan, h->shape.wave(), sw);
    if ((rc = load_route_big(h, plan, b, sw))) return rc;

    double *d_lut_eta = nullptr;
    rc = load_upload(h, plan, b, &d_lut_eta);
    if (!rc) rc = load_build_tables(h);
    if (!rc) rc = load_alloc_state(h, plan.SD);
    if (!rc) rc = load_params(h, d_lut_eta, v2p);
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the plan's vectors and v2p are free to die from here

    h->E = plan.E; h->M = plan.M; h->scn_off = 0; h->T = plan.T; h->C = plan.C; h->npc = plan.npc; h->P = plan.P; h->R = plan.R; h->D = plan.D; h->S = plan.S;
    if ((rc = load_decide_inl_stats(h, sw))) return rc;
    if ((rc = load_balance(h, b, sw))) return rc;
    // host mirrors for peek / stats / refill
    h->slot_port = std::move(plan.slot_port);
    h->port_slot = std::move(plan.port_slot);
    h->env_sess_start.assign(b->env_session_start, b->env_session_start + plan.M + 1);
    h->host_to_dev = std::move(plan.host_to_dev);
    h->sess_port = std::move(plan.sess_port);
    h->sess_afap = std::move(plan.sess_afap_host);
    h->cls_map = std::move(plan.cls_map);
    h->cs_vk_host = std::move(plan.cs_vk);
    h->cs_ph_host.assign(b->cs_phases, b->cs_phases + plan.C);
    h->cs_imax_host.assign(b->cs_max_charge_current, b->cs_max_charge_current + plan.C);
    h->refilled = false; h->load_gen += 1;
    h->loaded = true;
    if (h->extras.cost || h->extras.obs_f32 || h->extras.actions_f32) {
        const ev2g_step_extras keep = h->extras;
        if ((rc = ev2g_set_step_extras(h, &keep))) return rc;
    }
    return ev2g_reset_ex(h, nullptr, 0);
}

int ev2g_reset_ex(ev2g_handle *h, double *obs, int64_t scenario_offset) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_reset: no scenarios loaded");
    (void)hipSetDevice(h->device);
    const DevScn &s = h->scn;
    long long off = scenario_offset % (long long)s.M;
    if (off < 0) off += s.M;
    h->scn_off = off;
    // (the usage | potential | overload history slab is cleared by the reset kernel itself)
    if (h->st.cs_power_hist) {
        HIPCHK(h, hipMemsetAsync(h->st.cs_power_hist, 0, sizeof(double) * (size_t)s.T * s.E * s.C, h->stream));
        HIPCHK(h, hipMemsetAsync(h->st.cs_cur_hist, 0, sizeof(double) * (size_t)s.T * s.E * s.C, h->stream));
    }
    hipLaunchKernelGGL(ev2g_reset_kernel, dim3(s.n_groups), dim3(EV2G_BLOCK), 0, h->stream, s, h->st, obs, h->extras.obs_f32, (int)off);
    HIPCHK(h, hipGetLastError());
    h->current_step = 0;
    state_changed(h, "the episode was reset");
    return EV2G_OK;
}

int ev2g_reset(ev2g_handle *h, double *obs) { return ev2g_reset_ex(h, obs, h ? h->scn_off : 0); }
int ev2g_reset_f32(ev2g_handle *h, float *obs32, int64_t scenario_offset) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_reset: no scenarios loaded");
    const ev2g_step_extras keep = h->extras;
    if (obs32) h->extras.obs_f32 = obs32;   // (the reset kernel writes the float32 observation where the extras point; only the host-side copy changes here)
    const int rc = ev2g_reset_ex(h, nullptr, scenario_offset);
    h->extras = keep;
    return rc;
}
int64_t ev2g_scenario_offset(const ev2g_handle *h) { return h ? h->scn_off : 0; }
int ev2g_n_scenarios(const ev2g_handle *h) { return h ? h->M : 0; }

int ev2g_set_step_extras(ev2g_handle *h, const ev2g_step_extras *x) {
    if (!h) return EV2G_ERR_ARG;
    if (x && x->cost && h->cfg.cost_kind == EV2G_COST_NONE)
        return fail(h, EV2G_ERR_ARG, "ev2g_set_step_extras: a cost buffer needs ev2g_config.cost_kind != EV2G_COST_NONE");
    h->extras = x ? *x : ev2g_step_extras{};
    if (h->loaded && h->d_v2p) {   // refresh the extras inside the device-resident parameter block (stream-ordered)
        (void)hipSetDevice(h->device);
        struct { void *cost; long long cs; void *o32; long long os; const void *a32; } blk{
            h->extras.cost, h->extras.cost_step_stride, h->extras.obs_f32, h->extras.obs_f32_step_stride, h->extras.actions_f32};
        static_assert(sizeof(blk) == sizeof(V2P) - offsetof(V2P, x_cost), "StepExtras block is the tail of V2P");
        HIPCHK(h, hipMemcpyAsync((char *)h->d_v2p + offsetof(V2P, x_cost), &blk, sizeof blk, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));   // `blk` is a stack temporary
    }
    return EV2G_OK;
}

// the float64 blocks of one launch: the rows of its first step, and the strides the kernel advances them by from step to step
struct StepRows {
    Rows<const double> actions;
    Rows<double> obs, reward;
    Rows<uint8_t> done, mask;
    StepRows from(long long i) const {   // the same blocks, from row i on
        return {{actions.at(i), actions.stride}, {obs.at(i), obs.stride}, {reward.at(i), reward.stride}, {done.at(i), done.stride}, {mask.at(i), mask.stride}};
    }
};

// StepIO of one launch: the caller's buffers plus the scenario-pool window; step0 offsets the sticky extras' step strides
static StepIO make_io(const ev2g_handle *h, const StepRows &r, long long step0, int auto_reset) {
    StepIO io{};
    io.actions = r.actions.p; io.a_stride = r.actions.stride;
    io.obs = r.obs.p; io.o_stride = r.obs.stride;
    io.reward = r.reward.p; io.r_stride = r.reward.stride;
    io.done = r.done.p; io.d_stride = r.done.stride;
    io.mask = r.mask.p; io.m_stride = r.mask.stride;
    io.scn_off = (int)h->scn_off;
    io.scn_stride = (auto_reset == EV2G_AUTO_RESET_NEXT) ? h->E % h->M : 0;
    io.step0 = (int)step0;
    io.log_soc = (h->cfg.flags & EV2G_FLAG_LOG_SOC) ? 1 : 0;
    io.act32 = r.actions.p ? nullptr : h->extras.actions_f32;
    io.obs32 = (h->extras.obs_f32 && h->extras.obs_f32_step_stride == 0) ? h->extras.obs_f32 : nullptr;
    return io;
}

// One step launch: route_step (ev2g_route_host.h) decides from the loaded shape and from what this call passes, the decision is stored for the
// reporters and for launch_stats, and its table entry is launched.  `open_timing`: the launch is the whole of a timed call whose slot is taken
// (ev2g_step_n's single persistent launch) -- an accepted launch of an ev2g_step_wave instantiation with the stamp sites (StepRoute::stamps) gets the
// slot's stamp pair, any other one the opening event.
static int launch_steps(ev2g_handle *h, const StepIO &io, int t0, int k, int auto_reset, bool open_timing = false) {
    const DevScn &s = h->scn;
    const ev2g_step_extras &x = h->extras;
    h->state_epoch += 1;
    RouteCall c;
    c.actions = io.actions != nullptr; c.act32 = io.act32 != nullptr; c.obs = io.obs != nullptr; c.obs32 = io.obs32 != nullptr;
    c.reward = io.reward != nullptr; c.done = io.done != nullptr; c.mask = io.mask != nullptr;
    c.a_stride = io.a_stride; c.o_stride = io.o_stride; c.r_stride = io.r_stride; c.d_stride = io.d_stride; c.m_stride = io.m_stride;
    c.x_cost = x.cost != nullptr; c.x_obs_f32 = x.obs_f32 != nullptr; c.x_actions_f32 = x.actions_f32 != nullptr;
    c.x_cost_stride = x.cost_step_stride; c.x_obs_f32_stride = x.obs_f32_step_stride;
    c.t0 = t0; c.k = k; c.auto_reset = auto_reset;
    const StepRoute r = route_step(h->shape, c);
    if (r.refusal) {   // (nothing ran: the specialisation and its reason stay those of the launch before; its side results are gone all the same)
        h->last.inl_stats = false; h->last.ff = false; h->last.balance = false; h->last.inl_reason = r.inl_reason; h->last.balance_reason = "the launch was refused";
        return fail(h, EV2G_ERR_ARG, r.refusal);
    }
    h->last = r;
    unsigned long long *stamp = nullptr;
    if (open_timing) {
        if (r.family == ROUTE_WAVE && r.stamps && stamps_usable(h)) stamp = timed_stamps(h);
        else if (int rc = timed_events(h)) return rc;
    }
    const V2P *pp = (const V2P *)h->d_v2p;
    const LaunchDims d{dim3(s.n_groups), h->lds_bytes, h->stream};
    switch (r.family) {
    case ROUTE_WAVE: {
        const DevState &st = h->st;
        const int *grp_map = r.balance ? balance_get(h, h->scn_off) : nullptr;   // (the window's map: built at load, or here at a window's first launch)
        if (r.balance && !grp_map) { h->last.balance = false; h->last.balance_reason = "the window's map could not be copied to the device"; }
        const WaveArgs wa{s.P, s.T, s.E, s.D, s.M, st.slab_port, st.slab_port_slice, st.hist,
                    st.env_acc, s.cs_pack, (char *)st.line, h->d_step_tab, (char *)st.port_dyn, s.dict, h->shape.epw, s.P, grp_map, stamp};
        const WaveLaunch launch = kWaveTable[route_wave_index(r.sk, r.rk, r.io32, r.fullk)];
        if (!launch) return fail(h, EV2G_ERR_ARG, "EV2G_ONLY_00 build: only the cfg2 specialisation exists");   // (every entry a route names exists in a full build: tests/host/route_check.cpp)
        if (r.ff && h->d_place) HIPCHK(h, hipMemsetAsync(h->d_place, 0, sizeof(unsigned) * (2 * (size_t)s.n_groups + 2048), h->stream));   // (EV2G_PLACEMENT=1 only)
        launch(d, pp, io, t0, k, auto_reset, wa);
    } break;
    case ROUTE_BIG:
        hipLaunchKernelGGL(ev2g_step_big<EV2G_BIG_BLOCK>, dim3(s.E), dim3(EV2G_BIG_BLOCK), h->lds_big, h->stream, pp, io, t0, k, h->big_args);
        break;
    case ROUTE_V2:
        v2_kernel(r.block, r.spec).launch(d, pp, io, t0, k, auto_reset);
        break;
    default:
        hipLaunchKernelGGL(ev2g_step_kernel, d.grid, dim3(EV2G_BLOCK), d.lds, d.stream, s, h->st, io,
                           StepExtras{x.cost, x.cost_step_stride, x.obs_f32, x.obs_f32_step_stride, x.actions_f32}, t0, k, auto_reset);
    }
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

// ---- one-step launch chains ----
// What an entry that runs k x (stages around a one-step launch) asks for, in launch order: chain_steps enqueues it, run_chain is the whole timed
// call of a segment inside one episode (both stand below the stages they launch, behind grid_state_check).
struct StepChain {
    const char *who = "";   // the entry's name, for messages
    // the step's actions: the caller's rows; an agent that writes them (no rows: into its own block); or an actor's forward pass between the
    // float32 rows of the link or of the grid, whose fail / widen kernel makes the float64 block the step reads -- without either, between the
    // registered hand-over pair (ev2g_set_step_extras), which the step kernel reads itself
    Rows<double> actions;
    ev2g_heuristic *agent = nullptr;
    const ev2g_mlp *actor = nullptr;
    // a link: ahead of the step the fail kernel (p_fail > 0, and always under an actor), behind it the delay kernel (p_delay > 0) or, under an
    // actor, the plain float32 copy of the observation
    ev2g_link *link = nullptr;
    // a grid: behind the step the compose kernel, then (observed) the state kernel of the next step counter
    ev2g_grid *grid = nullptr;
    double base_weight = 0.0, voltage_weight = 0.0;
    bool observed = false;
    Rows<double> vm, gobs;
    Rows<float> gobs32;
    // an action wrapper (not with a link or a grid): between the action source and the step, from the caller's row -- under an actor from the
    // registered float32 action row -- into the wrapper's own float64 block or the caller's `wrapped` row, which the step then reads
    ev2g_wrap *wrap = nullptr;
    Rows<double> wrapped;
    // a Gaussian actor-critic (not with a link, a grid or a wrapper): its sampling launch reads float32 observation row i of ac_obs and writes the
    // sample, value and log-probability rows; the step reads the object's clipped block and writes observation row i + 1 -- per launch on the fast
    // path (ac_direct), through the registered hand-over pair with device-to-device copies elsewhere (ev2g_collect's two routes)
    ev2g_acpolicy *ac = nullptr;
    bool ac_deterministic = false, ac_direct = false;
    Rows<float> ac_obs, ac_actions, ac_values, ac_log_probs;
    // an ARS learner (not with a link, a grid or a wrapper): its population (or centre) launch reads the object's float32 observation row and
    // writes its action row; the step reads that row and writes the next observation over the first -- per launch on the fast path (ars_direct),
    // through the registered hand-over pair with device-to-device copies elsewhere, as the actor-critic's stage
    ev2g_ars *ars = nullptr;
    bool ars_population = false, ars_direct = false;
    Rows<double> obs, reward;   // every step's outputs
    Rows<uint8_t> done, mask;
    int auto_reset = 0;                // an episode end inside the segment (chain_steps; run_chain refuses it up front): 0 ends the call with EV2G_ERR_DONE
    bool a_stride_to_kernel = false;   // ev2g_step_n: StepIO::a_stride = actions.stride (the float32 action hand-over applies step0 * a_stride in the kernel)
    bool count_steps = true;           // StepIO::step0 = the step's index in the segment, else 0
};
static int chain_steps(ev2g_handle *h, const StepChain &c, int k);
static int run_chain(ev2g_handle *h, StepChain c, int k);
static int wrap_launch(ev2g_handle *h, ev2g_wrap *w, const void *in, bool in32, double *out);
static int ac_launch(ev2g_handle *h, ev2g_acpolicy *ac, const float *x, int n_rows, bool sample, float *mean, float *actions, float *clipped,
                     float *value, float *log_prob);
static int ars_launch(ev2g_handle *h, ev2g_ars *a, const float *x, int n_rows, bool population, float *actions);

int ev2g_step(ev2g_handle *h, const double *actions, double *obs, double *reward, uint8_t *done, uint8_t *action_mask) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_step: no scenarios loaded");
    if (!actions && !h->extras.actions_f32) return fail(h, EV2G_ERR_ARG, "ev2g_step: actions is null (and no float32 actions are set)");
    if (h->current_step >= h->T)
        return fail(h, EV2G_ERR_DONE, "ev2g_step: episode is done, reset the environment (ev2gym_env.py:343)");
    (void)hipSetDevice(h->device);
    const StepIO io = make_io(h, StepRows{{actions}, {obs}, {reward}, {done}, {action_mask}}, 0, 0);
    int rc = launch_steps(h, io, h->current_step, 1, 0);
    if (rc) return rc;
    h->current_step += 1;
    h->ring.untimed();
    return EV2G_OK;
}

int ev2g_step_n(ev2g_handle *h, int k_steps, int mode, const double *actions, int64_t a_stride, double *obs,
                int64_t o_stride, double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask,
                int64_t m_stride, int auto_reset) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_step_n: no scenarios loaded");
    if ((!actions && !h->extras.actions_f32) || k_steps < 0) return fail(h, EV2G_ERR_ARG, "ev2g_step_n: bad arguments");
    (void)hipSetDevice(h->device);
    int rc = EV2G_OK;
    const long long adv = (auto_reset == EV2G_AUTO_RESET_NEXT) ? h->E % h->M : 0;   // pool offset advance per in-run reset
    const StepRows rows{{actions, a_stride}, {obs, o_stride}, {reward, r_stride}, {done, d_stride}, {mask, m_stride}};
    // the call's slot of the timing ring; how it is timed is decided where the call knows what it launches: a persistent call that is ONE launch
    // leaves it to launch_steps (stamps where the instantiation has them), everything else -- the per-step chain, the run cut at the episode ends, a call of no
    // steps -- amortises one event pair over its launches
    h->ring.take();
    if (mode == EV2G_STEPN_PERSISTENT) {
        int k = k_steps;
        if (!auto_reset) k = std::min(k, h->T - h->current_step);
        // Per-session results (sess_final_cap, sess_abs_e) are indexed by pool session.  Two envs that run the same scenario inside
        // ONE launch store to the same slots from different XCDs, whose L2s are written back at the kernel boundary in no defined
        // order, so a launch covers several AUTO_RESET_NEXT episodes only while their windows are disjoint: (resets + 1) * E <= M.
        // Otherwise the run is cut at the episode ends (one launch per episode, host-side reset in between).
        int resets = 0;
        { int t = h->current_step; for (int i = 0; i < k; i++) { if (t >= h->T) { t = 0; resets++; } t++; } }
        if (adv != 0 && resets > 0 && (long long)(resets + 1) * h->E > h->M) {
            if ((rc = timed_events(h))) return rc;
            for (int i0 = 0; i0 < k;) {
                if (h->current_step >= h->T) {
                    int r2 = ev2g_reset_ex(h, nullptr, h->scn_off + adv);
                    if (r2) return r2;
                }
                const int kc = std::min(k - i0, h->T - h->current_step);
                int r2 = launch_steps(h, make_io(h, rows.from(i0), i0, 0), h->current_step, kc, 0);
                if (r2) return r2;
                h->current_step += kc;
                i0 += kc;
            }
            return timed_close(h);
        }
        rc = k > 0 ? launch_steps(h, make_io(h, rows, 0, auto_reset), h->current_step, k, auto_reset, true) : timed_events(h);
        if (rc) return rc;
        if (auto_reset) {
            // replay the step counter on the host: reset happens lazily before the step that follows a terminal one
            int t = h->current_step;
            for (int i = 0; i < k; i++) { if (t >= h->T) { t = 0; h->scn_off = (h->scn_off + adv) % h->M; } t++; }
            h->current_step = t;
        } else {
            h->current_step += k;
        }
        if (k < k_steps) rc = fail(h, EV2G_ERR_DONE, "ev2g_step_n: episode finished before k_steps (auto_reset off)");
    } else {
        if ((rc = timed_events(h))) return rc;
        StepChain c{"ev2g_step_n"};
        c.actions = {const_cast<double *>(actions), a_stride}; c.a_stride_to_kernel = true;   // (no agent: the rows are only read)
        c.obs = rows.obs; c.reward = rows.reward; c.done = rows.done; c.mask = rows.mask;
        c.auto_reset = auto_reset;
        rc = chain_steps(h, c, k_steps);
        if (rc && rc != EV2G_ERR_DONE) return rc;   // (an episode end with auto_reset off: the steps before it are a timed call)
    }
    const int rc2 = timed_close(h);
    return rc2 ? rc2 : rc;
}

// ---- policy in the loop -------------------------------------------------------------------------------------------
struct ev2g_mlp {
    MlpDev dev{};
    std::vector<void *> allocs;
    MlpPlan plan;               // the kernel for this shape and what a launch of it takes (ev2g_policy_host.h)
    const void *fn = nullptr, *fn_big = nullptr;   // kMlpTable[plan.index], kMlpTable[plan.big_index] (null: no 32-row variant)
    int big_from = 0;           // the 32-row variant runs batches of at least this many rows: more than 16 x CUs
    std::string kernel_name;    // ev2g_mlp_kernel_name
    ev2g_td3 *learner = nullptr;   // the TD3 / DDPG learner bound to this policy (ev2g_td3_create), destroyed with it
};
// (a learner leaves its policy first)
static void td3_free(ev2g_td3 *t) {
    if (t->policy) t->policy->learner = nullptr;
    release_owned(t);
}

extern "C++" {   // (templates: C++ linkage inside the C-ABI block)
// the actor kernels (MlpPlan::index / big_index): the table's order is mlp_table_key's
template <int I>
static const void *mlp_entry() {
    constexpr MlpKey K = mlp_table_key(I);
    if constexpr (K.kind == MLP_KIND_ANY) return (const void *)ev2g_mlp3_any;
    else if constexpr (K.kind == MLP_KIND_F32) return (const void *)ev2g_mlp3_f32;
    else if constexpr (K.kind == MLP_KIND_FIXED) {
        static_assert(mlp_fixed_index(K.a, K.b, K.c) == I, "the table's order is mlp_fixed_index's");
        return (const void *)ev2g_mlp3_fixed<K.a, K.b, K.c>;
    } else {
        static_assert(mlp_s16_index(K.a == 6 ? 0 : 1, K.nw, K.rb) == I, "the table's order is mlp_s16_index's");
        return (const void *)ev2g_mlp3_s16<K.a, K.b, K.c, K.d, K.nw, K.wv, K.rb>;
    }
}
template <size_t... I>
static std::array<const void *, sizeof...(I)> mlp_table(std::index_sequence<I...>) { return {mlp_entry<(int)I>()...}; }
static const std::array<const void *, MLP_TABLE_ENTRIES> kMlpTable = mlp_table(std::make_index_sequence<MLP_TABLE_ENTRIES>{});
}

// the device stage of a policy: uploads the plan's images, sets the kernels' dynamic-LDS attributes and drains the stream (the images are temporaries)
static int mlp_upload(ev2g_handle *h, ev2g_mlp *m, const MlpImages &img) {
    MlpDev &d = m->dev;
    const MlpPlan &p = m->plan;
#ifdef EV2G_MLP_TIMING
    if (int rc = dalloc(h, m->allocs, 16, &d.dbg)) return rc;
#endif
    const uint16_t **w[3] = {&d.w1, &d.w2, &d.w3};
    const float **b[3] = {&d.b1, &d.b2, &d.b3};
    for (int i = 0; i < 3; i++) {
        char *q = nullptr;
        if (int rc = upload(h, m->allocs, (const char *)img.weight(i), img.weight_bytes(i), &q)) return rc;
        *w[i] = (const uint16_t *)q;
    }
    for (int i = 0; i < 3; i++) {   // (the streaming kernel's biases are one array: layers 2 and 3 point into it)
        float *q = nullptr;
        if (img.bias[i].empty()) { *b[i] = d.b1 + img.bias_off[i]; continue; }
        if (int rc = upload(h, m->allocs, img.bias[i].data(), img.bias[i].size(), &q)) return rc;
        *b[i] = q;
    }
    if (p.lds > 48 * 1024) HIPCHK(h, hipFuncSetAttribute(m->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    if (m->fn_big && p.big_lds > 48 * 1024) HIPCHK(h, hipFuncSetAttribute(m->fn_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.big_lds));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

int ev2g_mlp_create_ex(ev2g_handle *h, int d_in, int h1, int h2, int d_out, const float *W1, const float *b1, const float *W2,
                    const float *b2, const float *W3, const float *b3, float out_lo, int precision, ev2g_mlp **out) {
    if (!h || !out || !W1 || !b1 || !W2 || !b2 || !W3 || !b3) return fail(h, EV2G_ERR_ARG, "ev2g_mlp_create: bad arguments");
    const MlpPlan p = plan_mlp(d_in, h1, h2, d_out, out_lo, precision);
    if (p.err) return fail(h, p.err, p.refusal);
    (void)hipSetDevice(h->device);
    ev2g_mlp *m = new ev2g_mlp();
    m->plan = p;
    MlpDev &d = m->dev;
    d.d_in = d_in; d.h1 = h1; d.h2 = h2; d.d_out = d_out;
    d.k1 = p.k1; d.n1 = p.n1; d.n2 = p.n2; d.n3 = p.n3;
    d.out_lo = out_lo;
    d.dbg = nullptr;
    m->fn = kMlpTable[(size_t)p.index];
    m->kernel_name = mlp_kernel_name(p.index);
    if (p.big_index >= 0) {
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
        m->fn_big = kMlpTable[(size_t)p.big_index];
        m->big_from = EV2G_MLPS_ROWS * cus + 1;
        m->kernel_name += "; from " + std::to_string(m->big_from) + " rows " + mlp_kernel_name(p.big_index);
    }
    if (const int rc = mlp_upload(h, m, pack_mlp(p, W1, b1, W2, b2, W3, b3))) {   // the one cleanup path
        (void)hipStreamSynchronize(h->stream);   // (copies of the images enqueued before the failure)
        free_pool(m->allocs);
        delete m;
        return rc;
    }
    *out = m;
    return EV2G_OK;
}

int ev2g_mlp_create(ev2g_handle *h, int d_in, int h1, int h2, int d_out, const float *W1, const float *b1, const float *W2,
                    const float *b2, const float *W3, const float *b3, float out_lo, ev2g_mlp **out) {
    return ev2g_mlp_create_ex(h, d_in, h1, h2, d_out, W1, b1, W2, b2, W3, b3, out_lo, EV2G_MLP_BF16, out);
}

void ev2g_mlp_destroy(ev2g_handle *h, ev2g_mlp *m) {
    if (!m) return;
    if (h && m->learner) owned_destroy(h, &ev2g_handle::td3s, m->learner, td3_free);   // (clears m->learner when `h` owns it)
    // no handle, or not the learner's: the learner stays its handle's, without a policy -- its entries then refuse (td3_check), its images are gone
    if (m->learner) m->learner->policy = nullptr;
    if (h) { (void)hipSetDevice(h->device); (void)hipStreamSynchronize(h->stream); drop_rollout_graphs(h); }
    free_pool(m->allocs);
    delete m;
}

int ev2g_mlp_forward(ev2g_handle *h, const ev2g_mlp *m, const float *x, float *y, int n_rows) {
    if (!h || !m || !x || !y || n_rows <= 0) return fail(h, EV2G_ERR_ARG, "ev2g_mlp_forward: bad arguments");
    (void)hipSetDevice(h->device);
    MlpDev dev = m->dev;
    void *args[] = {&dev, &x, &y, &n_rows};
    const MlpPlan &p = m->plan;
    if (m->fn_big && n_rows >= m->big_from)
        HIPCHK(h, hipLaunchKernel(m->fn_big, dim3((n_rows + p.big_rows - 1) / p.big_rows), dim3(p.big_threads), args, p.big_lds, h->stream));
    else
        HIPCHK(h, hipLaunchKernel(m->fn, dim3((n_rows + p.rows - 1) / p.rows), dim3(p.threads), args, p.lds, h->stream));
    return EV2G_OK;
}

const char *ev2g_mlp_kernel_name(const ev2g_mlp *m) { return m ? m->kernel_name.c_str() : ""; }

#ifdef EV2G_MLP_TIMING
int ev2g_mlp_debug_stamps(ev2g_handle *h, const ev2g_mlp *m, unsigned long long *out8) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out8, m->dev.dbg, 128, hipMemcpyDeviceToHost));   // (16 stamps: 0..7 the phases, 8.. finer ones of the prologue)
    return 0;
}
#endif

// ---- one launch per rollout segment (round 5): ev2g_step_wave<.., 1024, true> evaluates the policy between the steps, inside the launch ----
// route_fused (ev2g_route_host.h) says whether the loaded shape and this policy get it, and which instantiation; EV2G_NO_FUSED=1 and (the
// float32 policy) EV2G_NO_FUSED_F32=1, read at every call, keep the two launches per step.
static FusedRoute fused_route(const ev2g_handle *h, const ev2g_mlp *m) {
    return route_fused(h->shape, h->extras.cost != nullptr, m->plan.s16,
                       std::getenv("EV2G_NO_FUSED") != nullptr, std::getenv("EV2G_NO_FUSED_F32") != nullptr);
}
// k steps from the current one; obs0: the [E, D] float32 rows the first forward reads; obs / act / reward / done / mask: the rows of the segment's first
// step with their step strides
static int launch_fused(ev2g_handle *h, const ev2g_mlp *m, const FusedRoute &fr, int k, const float *obs0, Rows<float> obs, Rows<float> act,
                        Rows<double> reward, Rows<uint8_t> done, Rows<uint8_t> mask) {
    const DevScn &s = h->scn;
    const DevState &st = h->st;
    const long long lim = 1ll << 32;
    state_changed(h, "the last launch was a policy-in-the-loop segment (ev2g_rollout / ev2g_collect)");
    h->last.ff = false; h->last.balance = false; h->last.balance_reason = "the last launch was a policy-in-the-loop segment";
    if (obs.stride * 4 >= lim || act.stride * 4 >= lim || reward.stride * 8 >= lim || done.stride >= lim || mask.stride >= lim || obs.stride < 0 ||
        act.stride < 0 || reward.stride < 0 || done.stride < 0 || mask.stride < 0)
        return fail(h, EV2G_ERR_ARG, "ev2g_collect / ev2g_rollout: a step stride is negative or reaches 4 GiB");
    StepIO io = make_io(h, StepRows{{nullptr, act.stride}, {nullptr, obs.stride}, reward, done, mask}, 0, 0);
    io.act32 = act.p; io.obs32 = obs.p;
    // round 6: PublicPST envs of at most 32 ports go TWO to a wavefront (32 policy rows per workgroup)
    const int ae = fr.ae;
    const WaveArgs wa{s.P, s.T, s.E, s.D, s.M, st.slab_port, st.slab_port_slice, st.hist, st.env_acc, s.cs_pack, (char *)st.line, h->d_step_tab, (char *)st.port_dyn, s.dict, ae, ae == 1 ? s.P : 32};
    FusedArgs fa{};
    fa.m = m->dev; fa.obs0 = obs0;
    const LaunchDims d{dim3((s.E + 16 * ae - 1) / (16 * ae)), ev2g_fused_lds_bytes(ae, fr.nwf), h->stream};
    const FusedEntry *e = (fr.index >= 0 && fr.index < ROUTE_FUSED_ENTRIES) ? &kFusedTable[(size_t)fr.index] : nullptr;
    if (!e || !e->fn) return fail(h, EV2G_ERR_STATE, "internal: no fused instantiation for this plugin pair");
    if (!(h->fused_attr_mask & (1u << fr.index))) {   // function attributes are per device: once per handle, not per process
        HIPCHK(h, hipFuncSetAttribute(e->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)d.lds));
        h->fused_attr_mask |= 1u << fr.index;
    }
    e->launch(d, (const V2P *)h->d_v2p, io, h->current_step, k, wa, fa);
    HIPCHK(h, hipGetLastError());
    h->last.specialisation = 4;
    h->last.general_reason = "";
    return EV2G_OK;
}

int ev2g_rollout(ev2g_handle *h, const ev2g_mlp *m, int k_steps, double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride,
                 uint8_t *mask, int64_t m_stride, int auto_reset) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_rollout: no scenarios loaded");
    if (!m || k_steps < 0) return fail(h, EV2G_ERR_ARG, "ev2g_rollout: bad arguments");
    const ev2g_step_extras &x = h->extras;
    if (!x.obs_f32 || !x.actions_f32 || x.obs_f32_step_stride != 0)
        return fail(h, EV2G_ERR_ARG, "ev2g_rollout: register float32 observation (step stride 0) and action buffers with ev2g_set_step_extras first");
    if (m->dev.d_in != h->D || m->dev.d_out != h->P) return fail(h, EV2G_ERR_ARG, "ev2g_rollout: actor shape != (obs dim, ports)");
    (void)hipSetDevice(h->device);
    // the k x (actor forward, env step) launches: the forward pass works on the registered float32 pair, which the step reads and writes itself
    StepChain c{"ev2g_rollout"};
    c.actor = m;
    c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    c.auto_reset = auto_reset;
    c.count_steps = x.cost != nullptr;   // (a cost buffer may record every step; the float32 buffers do not advance)
    if (int rc = timed_open(h)) return rc;
    int rc = EV2G_OK;
    static const bool use_graphs = [] { const char *e = std::getenv("EV2G_ROLLOUT_GRAPHS"); return !(e && e[0] == '0'); }();
    const bool whole = h->current_step + k_steps <= h->T;   // no episode end inside the segment: nothing but kernel launches
    const FusedRoute fr = (whole && k_steps >= 1 && reward && done && mask) ? fused_route(h, m) : FusedRoute{};
    if (fr.eligible) {   // ONE launch: the policy between the steps, inside it
        rc = launch_fused(h, m, fr, k_steps, x.obs_f32, {x.obs_f32}, {(float *)x.actions_f32}, c.reward, c.done, c.mask);
        if (rc) return rc;
        h->current_step += k_steps;
    } else
    if (use_graphs && whole && k_steps >= 4) {
        ev2g_handle::RolloutGraph *hit = nullptr;
        for (auto &g : h->rollout_graphs)
            if (g.mlp == m && g.k == k_steps && g.t0 == h->current_step && g.scn_off == h->scn_off && g.rew == reward && g.done == done &&
                g.mask == mask && g.rs == r_stride && g.ds == d_stride && g.ms == m_stride && std::memcmp(&g.x, &x, sizeof x) == 0) { hit = &g; break; }
        if (!hit) {
            const int t_before = h->current_step;
            hipGraph_t graph = nullptr;
            HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            rc = chain_steps(h, c, k_steps);   // (no episode end inside: nothing but kernel launches)
            const hipError_t ce = hipStreamEndCapture(h->stream, &graph);
            h->current_step = t_before;
            if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
            if (ce != hipSuccess) return fail(h, EV2G_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
            hipGraphExec_t exec = nullptr;
            const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) return fail(h, EV2G_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
            if (h->rollout_graphs.size() >= 64) {   // bounded cache: drop the oldest
                (void)hipGraphExecDestroy(h->rollout_graphs.front().exec);
                h->rollout_graphs.erase(h->rollout_graphs.begin());
            }
            h->rollout_graphs.push_back({m, k_steps, t_before, h->scn_off, reward, done, mask, r_stride, d_stride, m_stride, x, exec});
            hit = &h->rollout_graphs.back();
        }
        HIPCHK(h, hipGraphLaunch(hit->exec, h->stream));
        h->current_step += k_steps;
        h->graph_launches++;
    } else {
        rc = chain_steps(h, c, k_steps);
    }
    const int rc2 = timed_close(h);   // (also behind a segment that ended early or failed in chain_steps: its launches are on the stream)
    return rc2 ? rc2 : rc;
}

long long ev2g_rollout_graph_launches(const ev2g_handle *h) { return h ? h->graph_launches : 0; }

// the collectors' route (ev2g_route_host.h) of this handle, as things are registered now
static bool collect_direct(const ev2g_handle *h) {
    const ev2g_step_extras &x = h->extras;
    return collect_direct(h->shape, x.cost != nullptr, x.obs_f32 != nullptr, x.actions_f32 != nullptr);
}

// The collectors' loop (ev2g_collect, ev2g_sac_collect): k_steps x (actor(observation row, action row, E rows) -> one-step launch) over the
// caller's transition rows.  `fused`: the policy whose eligible segments run as ONE launch, or null.
extern "C++" template <class Actor>
static int collect_rows(ev2g_handle *h, const char *who_c, int k_steps, const ev2g_transitions *tr, const ev2g_mlp *fused, Actor actor) {
    const std::string who(who_c);
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, who + ": no scenarios loaded");
    if (!tr || k_steps < 0 || !tr->obs || !tr->actions || !tr->reward || !tr->done || !tr->mask)
        return fail(h, EV2G_ERR_ARG, who + ": null argument (every transition array is required)");
    if (h->current_step + k_steps > h->T) return fail(h, EV2G_ERR_DONE, who + ": the segment would run past the episode end");
    (void)hipSetDevice(h->device);
    const size_t ED = (size_t)h->E * h->D, EP = (size_t)h->E * h->P;
    // On the fast path the policy hand-over instantiations take their float32 buffers per launch (StepIO::act32 / obs32): every step
    // reads and writes the caller's rows directly.  Elsewhere (general kernels; run-time rewards; a registered cost buffer) the step
    // works on the registered hand-over buffers of ev2g_set_step_extras and the rows are copied device-to-device around it.
    const ev2g_step_extras &x = h->extras;
    const bool direct = collect_direct(h);
    if (!direct && !(x.obs_f32 && x.actions_f32 && x.obs_f32_step_stride == 0))
        return fail(h, EV2G_ERR_ARG, who + ": this configuration steps through the registered float32 hand-over buffers: register them with "
                                     "ev2g_set_step_extras (observation step stride 0) first");
    const Rows<float> obs{tr->obs, (long long)ED}, act{tr->actions, (long long)EP};
    const Rows<double> reward{tr->reward, h->E};
    const Rows<uint8_t> done{tr->done, h->E}, mask{tr->mask, (long long)EP};
    if (int rc = timed_open(h)) return rc;
    const FusedRoute fr = (fused && direct && k_steps >= 1) ? fused_route(h, fused) : FusedRoute{};
    if (fr.eligible) {   // ONE launch for the segment: rows read and written in place, the policy inside the launch
        const int rc = launch_fused(h, fused, fr, k_steps, tr->obs, {obs.at(1), obs.stride}, act, reward, done, mask);
        if (rc) return rc;
        h->current_step += k_steps;
        k_steps = 0;
    }
    for (int i = 0; i < k_steps; i++) {
        float *obs_i = obs.at(i), *obs_n = obs.at(i + 1), *act_i = act.at(i);
        StepIO io = make_io(h, StepRows{{}, {}, {reward.at(i)}, {done.at(i)}, {mask.at(i)}}, 0, 0);
        int rc;
        if (direct) {
            if ((rc = actor(obs_i, act_i, h->E))) return rc;
            io.act32 = act_i; io.obs32 = obs_n;
            if ((rc = launch_steps(h, io, h->current_step, 1, 0))) return rc;
            if (h->last.specialisation <= 0) return fail(h, EV2G_ERR_STATE, who + ": internal: the direct path needs the full instantiation");
        } else {
            if (i == 0) HIPCHK(h, hipMemcpyAsync(x.obs_f32, obs_i, ED * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
            if ((rc = actor((const float *)x.obs_f32, (float *)x.actions_f32, h->E))) return rc;
            if ((rc = launch_steps(h, io, h->current_step, 1, 0))) return rc;
            HIPCHK(h, hipMemcpyAsync(act_i, x.actions_f32, EP * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(obs_n, x.obs_f32, ED * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        }
        h->current_step += 1;
    }
    return timed_close(h);
}

int ev2g_collect(ev2g_handle *h, const ev2g_mlp *m, int k_steps, const ev2g_transitions *tr) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_collect: no scenarios loaded");
    if (!m || !tr || k_steps < 0 || !tr->obs || !tr->actions || !tr->reward || !tr->done || !tr->mask)   // (ahead of the actor's shape, as ever)
        return fail(h, EV2G_ERR_ARG, "ev2g_collect: null argument (every transition array is required)");
    if (m->dev.d_in != h->D || m->dev.d_out != h->P) return fail(h, EV2G_ERR_ARG, "ev2g_collect: actor shape != (obs dim, ports)");
    return collect_rows(h, "ev2g_collect", k_steps, tr, m, [&](const float *obs, float *act, int n) { return ev2g_mlp_forward(h, m, obs, act, n); });
}

// ---- env-reading heuristic agents (ev2g_heuristic.h) ----
// what an agent kind needs of the loaded scenarios beyond their envs and ports; asked at create and again before every launch, because
// ev2g_load_scenarios may replace the scenarios under a live agent (same E and P, other chargers)
static int heuristic_shape_check(ev2g_handle *h, int kind, const std::string &who) {
    const bool gf = kind == EV2G_AGENT_ROUND_ROBIN_GF || kind == EV2G_AGENT_ROUND_ROBIN_GF_OFF_ALLOWED;
    // the reference indexes its per-charger max_cs_power with a port id (heuristics.py:392): it is defined for one-port chargers only
    // (and the kernel reads the charger table with that port id)
    if (gf && h->P != h->C)
        return fail(h, EV2G_ERR_ARG, who + ": RoundRobin_GF / RoundRobin_GF_off_allowed need one port per charger "
                                           "(the reference indexes its per-charger power table with a port id)");
    // one env's queue stage has to fit the 64 KiB of LDS
    if (gf && ev2g_heur_gf_wave_bytes(h->P) > 65536)
        return fail(h, EV2G_ERR_ARG, who + ": RoundRobin_GF / RoundRobin_GF_off_allowed support up to 3100 ports per env");
    if (kind == EV2G_HEURISTIC_ROUND_ROBIN && ev2g_heur_rr_wave_bytes(h->P) > 65536)
        return fail(h, EV2G_ERR_ARG, who + ": RoundRobin supports up to 13000 ports per env");
    return EV2G_OK;
}

// the device stage of an agent: its action block and, for the RoundRobin kinds, the queue
static int heuristic_device_stage(ev2g_handle *h, ev2g_heuristic *a) {
    const bool gf = a->kind == EV2G_AGENT_ROUND_ROBIN_GF || a->kind == EV2G_AGENT_ROUND_ROBIN_GF_OFF_ALLOWED;
    if (int rc = dalloc(h, a->allocs, (size_t)a->E * a->P, &a->act)) return rc;
    return a->kind == EV2G_HEURISTIC_ROUND_ROBIN || gf ? queue_alloc(h, a->allocs, a->E, a->P, gf, &a->q) : EV2G_OK;
}

int ev2g_heuristic_create(ev2g_handle *h, int kind, ev2g_heuristic **out) {
    if (!h || !out) return fail(h, EV2G_ERR_ARG, "ev2g_heuristic_create: null argument");
    *out = nullptr;
    if (!h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_heuristic_create: no scenarios loaded");
    if (kind < EV2G_HEURISTIC_CHARGE_AS_LATE_AS_POSSIBLE || kind > EV2G_AGENT_ROUND_ROBIN_GF_OFF_ALLOWED)
        return fail(h, EV2G_ERR_ARG, "ev2g_heuristic_create: unknown heuristic kind");
    if (int rc = heuristic_shape_check(h, kind, "ev2g_heuristic_create")) return rc;
    (void)hipSetDevice(h->device);
    ev2g_heuristic *a = new ev2g_heuristic();
    a->kind = kind; a->E = h->E; a->P = h->P;
    return owned_created(h, &ev2g_handle::heuristics, a, heuristic_device_stage(h, a), out);
}

void ev2g_heuristic_destroy(ev2g_handle *h, ev2g_heuristic *a) { owned_destroy(h, &ev2g_handle::heuristics, a); }

static int heuristic_check(ev2g_handle *h, ev2g_heuristic *a, const char *who) {
    if (int rc = owned_check(h, &ev2g_handle::heuristics, a, "heuristic", who)) return rc;
    if (a->E != h->E || a->P != h->P)
        return fail(h, EV2G_ERR_ARG, std::string(who) + ": the loaded scenarios' envs / ports differ from those the heuristic was created for");
    return heuristic_shape_check(h, a->kind, who);
}

// the agent's actions for the current step into actions [E, P] (device); the RoundRobin agents' queues advance
static int heuristic_launch(ev2g_handle *h, ev2g_heuristic *a, double *actions) {
    const DevScn &s = h->scn;
    const HeurArgs ha{h->d_port_slot, h->d_heur_cs_kw, h->heur_avg_power, a->q.queue, a->q.qlen, (int)h->scn_off,
                      h->d_heur_cs_min_kw, h->heur_min_action, a->q.qmin, a->q.qmax};
    const int t = h->current_step;
    if (a->kind == EV2G_AGENT_ROUND_ROBIN_GF || a->kind == EV2G_AGENT_ROUND_ROBIN_GF_OFF_ALLOWED) {
        // as RoundRobin below, with the two power lists in the stage
        const size_t wb = ev2g_heur_gf_wave_bytes(s.P);   // (<= 64 KiB: heuristic_shape_check)
        const int epb = (int)std::min<size_t>(EV2G_HEUR_BLOCK / 64, 65536 / wb);
        const dim3 grid((s.E + epb - 1) / epb), block(64 * epb);
        if (a->kind == EV2G_AGENT_ROUND_ROBIN_GF)
            hipLaunchKernelGGL(ev2g_heuristic_kernel<EV2G_HEUR_RRGF>, grid, block, epb * wb, h->stream, s, h->st, ha, t, actions);
        else
            hipLaunchKernelGGL(ev2g_heuristic_kernel<EV2G_HEUR_RRGF_OFF>, grid, block, epb * wb, h->stream, s, h->st, ha, t, actions);
    } else if (a->kind == EV2G_HEURISTIC_ROUND_ROBIN) {
        // one wavefront per env, up to four per workgroup while their LDS stages fit 64 KiB
        const size_t wb = ev2g_heur_rr_wave_bytes(s.P);   // (<= 64 KiB: heuristic_shape_check)
        const int epb = (int)std::min<size_t>(EV2G_HEUR_BLOCK / 64, 65536 / wb);
        hipLaunchKernelGGL(ev2g_heuristic_kernel<EV2G_HEUR_RR>, dim3((s.E + epb - 1) / epb), dim3(64 * epb), epb * wb, h->stream, s, h->st, ha,
                           t, actions);
    } else {
        const long long n = (long long)s.E * s.P;
        const dim3 grid((unsigned)((n + EV2G_HEUR_BLOCK - 1) / EV2G_HEUR_BLOCK));
        if (a->kind == EV2G_HEURISTIC_CHARGE_AS_LATE_AS_POSSIBLE)
            hipLaunchKernelGGL(ev2g_heuristic_kernel<EV2G_HEUR_CALP>, grid, dim3(EV2G_HEUR_BLOCK), 0, h->stream, s, h->st, ha, t, actions);
        else if (a->kind == EV2G_AGENT_CHARGE_AS_LATE_TO_DESIRED_CAPACITY)
            hipLaunchKernelGGL(ev2g_heuristic_kernel<EV2G_HEUR_CALPDC>, grid, dim3(EV2G_HEUR_BLOCK), 0, h->stream, s, h->st, ha, t, actions);
        else
            hipLaunchKernelGGL(ev2g_heuristic_kernel<EV2G_HEUR_CAFTDC>, grid, dim3(EV2G_HEUR_BLOCK), 0, h->stream, s, h->st, ha, t, actions);
    }
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_heuristic_actions(ev2g_handle *h, ev2g_heuristic *a, double *actions) {
    int rc = heuristic_check(h, a, "ev2g_heuristic_actions");
    if (rc) return rc;
    if (!actions) return fail(h, EV2G_ERR_ARG, "ev2g_heuristic_actions: actions is null");
    if (h->current_step >= h->T) return fail(h, EV2G_ERR_DONE, "ev2g_heuristic_actions: episode is done, reset the environment");
    return heuristic_launch(h, a, actions);
}

int ev2g_heuristic_run(ev2g_handle *h, ev2g_heuristic *a, int k_steps, double *actions, int64_t a_stride, double *obs, int64_t o_stride,
                       double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride) {
    if (int rc = heuristic_check(h, a, "ev2g_heuristic_run")) return rc;
    StepChain c{"ev2g_heuristic_run"};
    c.agent = a; c.actions = {actions, a_stride};
    c.obs = {obs, o_stride}; c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    return run_chain(h, c, k_steps);
}

// ---- communication-fault links (ev2g_link.h) ----
// a host matrix in the reference's layout [E, P, T] in the device's [T, E, P]
static std::vector<double> link_transposed(const double *src, int E, int P, int T) {
    std::vector<double> tr((size_t)E * P * T);
    for (int e = 0; e < E; e++)
        for (int p = 0; p < P; p++)
            for (int t = 0; t < T; t++) tr[((size_t)t * E + e) * P + p] = src[((size_t)e * P + p) * T + t];
    return tr;
}

// the device stage of a link: the held commands and the two energy columns (zero: what ev2g_link_reset_state leaves), the uniforms the caller
// gave (empty: none), and the stream drained behind their copies
static int link_device_stage(ev2g_handle *h, ev2g_link *l, const std::vector<double> &rand_act, const std::vector<double> &rand_obs) {
    for (double **b : {&l->held, &l->prev, &l->actual})
        if (int rc = dalloc(h, l->allocs, (size_t)l->E * l->P, b)) return rc;
    if (!rand_act.empty())
        if (int rc = upload(h, l->allocs, rand_act.data(), rand_act.size(), &l->rand_act)) return rc;
    if (!rand_obs.empty())
        if (int rc = upload(h, l->allocs, rand_obs.data(), rand_obs.size(), &l->rand_obs)) return rc;
    return drain(h);
}

int ev2g_link_create(ev2g_handle *h, double p_fail, double p_delay, uint64_t seed_act, uint64_t seed_obs, const double *rand_act,
                     const double *rand_obs, ev2g_link **out) {
    if (!h || !out) return fail(h, EV2G_ERR_ARG, "ev2g_link_create: null argument");
    *out = nullptr;
    if (!h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_link_create: no scenarios loaded");
    if (!(p_fail >= 0.0 && p_fail <= 1.0) || !(p_delay >= 0.0 && p_delay <= 1.0))
        return fail(h, EV2G_ERR_ARG, "ev2g_link_create: p_fail and p_delay must be between 0 and 1 (noise_wrappers.py:24,76)");
    if (p_delay > 0.0 && (h->cfg.state_kind != EV2G_STATE_PUBLIC_PST || h->D != 3 + 3 * h->P))
        return fail(h, EV2G_ERR_ARG, "ev2g_link_create: delayed observations need the PublicPST state function (noise_wrappers.py:79-80)");
    (void)hipSetDevice(h->device);
    ev2g_link *l = new ev2g_link();
    l->E = h->E; l->P = h->P; l->T = h->T;
    l->p_fail = p_fail; l->p_delay = p_delay; l->seed_act = seed_act; l->seed_obs = seed_obs;
    // (the copies' sources: they outlive the stage's drain, and the tail's behind a failure)
    std::vector<double> ta, to;
    if (rand_act && p_fail > 0.0) ta = link_transposed(rand_act, l->E, l->P, l->T);
    if (rand_obs && p_delay > 0.0) to = link_transposed(rand_obs, l->E, l->P, l->T);
    return owned_created(h, &ev2g_handle::links, l, link_device_stage(h, l, ta, to), out);
}

void ev2g_link_destroy(ev2g_handle *h, ev2g_link *l) { owned_destroy(h, &ev2g_handle::links, l); }

static int link_check(ev2g_handle *h, ev2g_link *l, const char *who) {
    if (int rc = owned_check(h, &ev2g_handle::links, l, "link", who)) return rc;
    if (l->E != h->E || l->P != h->P || l->T != h->T)
        return fail(h, EV2G_ERR_ARG, std::string(who) + ": the loaded scenarios' envs / ports / steps differ from those the link was created for");
    return EV2G_OK;
}

int ev2g_link_reset_state(ev2g_handle *h, ev2g_link *l) {
    if (int rc = link_check(h, l, "ev2g_link_reset_state")) return rc;
    const size_t EP = (size_t)l->E * l->P * sizeof(double);
    HIPCHK(h, hipMemsetAsync(l->held, 0, EP, h->stream));
    HIPCHK(h, hipMemsetAsync(l->prev, 0, EP, h->stream));
    HIPCHK(h, hipMemsetAsync(l->actual, 0, EP, h->stream));
    return EV2G_OK;
}

// one of the link's own blocks of n elements, allocated on first use
extern "C++" template <typename T>
static int link_buffer(ev2g_handle *h, ev2g_link *l, T **p, size_t n) {
    return *p ? EV2G_OK : dalloc(h, l->allocs, n, p);
}

// the fail kernel for step t: in [E, P] (float64, or float32 with in32) -> the link's held block, and `out` when given
static int link_launch_act(ev2g_handle *h, ev2g_link *l, int t, const void *in, bool in32, double *out) {
    const LinkRand r{l->rand_act, l->seed_act, l->E, l->P, l->T};
    const long long n = (long long)l->E * l->P;
    const dim3 grid((unsigned)std::min<long long>((n + EV2G_LINK_BLOCK - 1) / EV2G_LINK_BLOCK, 1 << 20));
    if (in32) hipLaunchKernelGGL(ev2g_link_act_kernel<true>, grid, dim3(EV2G_LINK_BLOCK), 0, h->stream, in, r, l->p_fail, t, l->held, out);
    else hipLaunchKernelGGL(ev2g_link_act_kernel<false>, grid, dim3(EV2G_LINK_BLOCK), 0, h->stream, in, r, l->p_fail, t, l->held, out);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

// the delay kernel on the observation of env step t (0 = the reset observation ... T = the terminal one)
static int link_launch_obs(ev2g_handle *h, ev2g_link *l, int t, double *obs, float *obs32) {
    const LinkRand r{l->rand_obs, l->seed_obs, l->E, l->P, l->T};
    const int epb = EV2G_LINK_BLOCK / 64;
    hipLaunchKernelGGL(ev2g_link_obs_kernel, dim3((l->E + epb - 1) / epb), dim3(EV2G_LINK_BLOCK), 0, h->stream, obs, obs32, r, l->p_delay, h->D, t,
                       (double)h->scn.dt, l->prev, l->actual);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_link_actions(ev2g_handle *h, ev2g_link *l, int t, const void *in, int in_is_f32, double *out) {
    if (int rc = link_check(h, l, "ev2g_link_actions")) return rc;
    if (!in) return fail(h, EV2G_ERR_ARG, "ev2g_link_actions: the action block is null");
    if (t < 0) t = h->current_step;
    if (t >= l->T) return fail(h, EV2G_ERR_DONE, "ev2g_link_actions: step " + std::to_string(t) + " is past the episode's last step");
    return link_launch_act(h, l, t, in, in_is_f32 != 0, out);
}

int ev2g_link_observe(ev2g_handle *h, ev2g_link *l, int t, double *obs, float *obs32) {
    if (int rc = link_check(h, l, "ev2g_link_observe")) return rc;
    if (!obs) return fail(h, EV2G_ERR_ARG, "ev2g_link_observe: the observation block is null");
    if (h->cfg.state_kind != EV2G_STATE_PUBLIC_PST || h->D != 3 + 3 * l->P)
        return fail(h, EV2G_ERR_ARG, "ev2g_link_observe: delayed observations need the PublicPST state function (noise_wrappers.py:79-80)");
    if (t < 0) t = h->current_step;
    if (t > l->T) return fail(h, EV2G_ERR_ARG, "ev2g_link_observe: step " + std::to_string(t) + " is past the terminal observation");
    return link_launch_obs(h, l, t, obs, obs32);
}

float *ev2g_link_obs_f32(ev2g_handle *h, ev2g_link *l) {
    if (link_check(h, l, "ev2g_link_obs_f32")) return nullptr;
    if (link_buffer(h, l, &l->obs32, (size_t)l->E * h->D)) return nullptr;
    return l->obs32;
}

int ev2g_link_run(ev2g_handle *h, ev2g_link *l, ev2g_heuristic *a, int k_steps, double *actions, int64_t a_stride, double *obs, int64_t o_stride,
                  double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride) {
    int rc = link_check(h, l, "ev2g_link_run");
    if (rc) return rc;
    if (a && (rc = heuristic_check(h, a, "ev2g_link_run"))) return rc;
    StepChain c{"ev2g_link_run"};
    c.agent = a; c.actions = {actions, a_stride};
    c.link = l;
    c.obs = {obs, o_stride}; c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    return run_chain(h, c, k_steps);
}

int ev2g_link_rollout(ev2g_handle *h, ev2g_link *l, const ev2g_mlp *m, int k_steps, double *reward, int64_t r_stride, uint8_t *done,
                      int64_t d_stride, uint8_t *mask, int64_t m_stride) {
    int rc = link_check(h, l, "ev2g_link_rollout");
    if (rc) return rc;
    if (!m || k_steps < 0 || r_stride < 0 || d_stride < 0 || m_stride < 0) return fail(h, EV2G_ERR_ARG, "ev2g_link_rollout: bad arguments");
    if (m->dev.d_in != h->D || m->dev.d_out != h->P) return fail(h, EV2G_ERR_ARG, "ev2g_link_rollout: actor shape != (obs dim, ports)");
    StepChain c{"ev2g_link_rollout"};
    c.actor = m;
    c.link = l;
    c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    return run_chain(h, c, k_steps);
}

// ---- distribution grid: the Laurent power flow after each step (ev2g_grid.h) ----
// the device stage of a grid: the network (kt: K transposed, n x n complex), the base profiles if any with the episode's voltage statistics
// (zero until the first step of an episode overwrites them), the per-env rows, and the stream drained behind the copies
static int grid_device_stage(ev2g_handle *h, ev2g_grid *g, const std::vector<double> &kt, const double *L, const double *p_base, const double *q_base) {
    const size_t n = (size_t)g->n, E = (size_t)g->E, prof = (size_t)g->M * (g->T + 1) * n;
    if (int rc = upload(h, g->allocs, (const double2 *)kt.data(), n * n, &g->Kt)) return rc;
    if (int rc = upload(h, g->allocs, (const double2 *)L, n, &g->L)) return rc;
    if (p_base) {
        if (int rc = upload(h, g->allocs, p_base, prof, &g->p_base)) return rc;
        if (int rc = upload(h, g->allocs, q_base, prof, &g->q_base)) return rc;
    }
    if (int rc = dalloc(h, g->allocs, E * (n + 1), &g->vm)) return rc;
    if (int rc = dalloc(h, g->allocs, E, &g->rew)) return rc;
    if (p_base) {
        for (double **b : {&g->vv_sum, &g->rew_sum})
            if (int rc = dalloc(h, g->allocs, E, b)) return rc;
        for (int **b : {&g->vv_count, &g->vv_steps})
            if (int rc = dalloc(h, g->allocs, E, b)) return rc;
    }
    return drain(h);
}

int ev2g_grid_create(ev2g_handle *h, int n_bus, const double *K, const double *L, double s_base, double tolerance, int max_iter,
                     const double *p_base, const double *q_base, ev2g_grid **out) {
    if (!h || !out) return fail(h, EV2G_ERR_ARG, "ev2g_grid_create: null argument");
    *out = nullptr;
    if (!h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_grid_create: no scenarios loaded");
    if (!K || !L) return fail(h, EV2G_ERR_ARG, "ev2g_grid_create: K or L is null");
    if (n_bus < 2 || max_iter < 0 || !(s_base > 0.0)) return fail(h, EV2G_ERR_ARG, "ev2g_grid_create: n_bus < 2, max_iter < 0 or s_base <= 0");
    const int n = n_bus - 1;
    if (ev2g_grid_wave_bytes(n) > EV2G_GRID_LDS_MAX) return fail(h, EV2G_ERR_ARG, "ev2g_grid_create: up to 1025 buses (one row's stage has to fit 48 KiB of LDS)");
    if ((p_base == nullptr) != (q_base == nullptr)) return fail(h, EV2G_ERR_ARG, "ev2g_grid_create: p_base and q_base come together");
    // the reference builds one transformer per non-slack bus (loaders.py:481-485) and writes node i + 1 from transformer i (ev2gym_env.py:388-390)
    if (p_base && h->R != n)
        return fail(h, EV2G_ERR_ARG, "ev2g_grid_create: the loaded scenarios have " + std::to_string(h->R) + " transformers, the grid needs n_bus - 1 = " +
                                     std::to_string(n) + " (one per non-slack bus, loaders.py:481-485)");
    (void)hipSetDevice(h->device);
    ev2g_grid *g = new ev2g_grid();
    g->E = h->E; g->T = h->T; g->M = h->M; g->n = n; g->max_iter = max_iter; g->s_base = s_base; g->tolerance = tolerance;
    std::vector<double> kt((size_t)n * n * 2);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            kt[((size_t)j * n + i) * 2] = K[((size_t)i * n + j) * 2];
            kt[((size_t)j * n + i) * 2 + 1] = K[((size_t)i * n + j) * 2 + 1];
        }
    return owned_created(h, &ev2g_handle::grids, g, grid_device_stage(h, g, kt, L, p_base, q_base), out);
}

void ev2g_grid_destroy(ev2g_handle *h, ev2g_grid *g) { owned_destroy(h, &ev2g_handle::grids, g); }

static int grid_check(ev2g_handle *h, ev2g_grid *g, bool run, const char *who) {
    if (int rc = owned_check(h, &ev2g_handle::grids, g, "grid", who)) return rc;
    if (run) {
        if (!g->p_base) return fail(h, EV2G_ERR_ARG, std::string(who) + ": the grid was created without base profiles (a solver only)");
        if (g->E != h->E || g->T != h->T || g->M != h->M || g->n != h->R)
            return fail(h, EV2G_ERR_ARG, std::string(who) + ": the loaded scenarios' envs / steps / pool / transformers differ from those the grid was created for");
    }
    return EV2G_OK;
}

// one wavefront per row, up to EV2G_GRID_WAVES per workgroup while their LDS stages fit the 48 KiB a launch gets without a function attribute
static int grid_launch(ev2g_handle *h, const ev2g_grid *g, GridArgs ga, bool compose) {
    if (ga.n_rows <= 0) return EV2G_OK;
    ga.Kt = g->Kt; ga.L = g->L; ga.n = g->n; ga.max_iter = g->max_iter; ga.s_base = g->s_base; ga.tolerance = g->tolerance;
    const size_t wb = ev2g_grid_wave_bytes(g->n);   // (<= EV2G_GRID_LDS_MAX: ev2g_grid_create)
    const int epb = (int)std::min<size_t>(EV2G_GRID_WAVES, EV2G_GRID_LDS_MAX / wb);
    const dim3 grid((ga.n_rows + epb - 1) / epb), block(64 * epb);
    if (compose) hipLaunchKernelGGL(ev2g_grid_kernel<true>, grid, block, epb * wb, h->stream, ga);
    else hipLaunchKernelGGL(ev2g_grid_kernel<false>, grid, block, epb * wb, h->stream, ga);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_grid_solve(ev2g_handle *h, ev2g_grid *g, const double *p_kw, const double *q_kw, int n_rows, double *vm, double *v_complex,
                    int32_t *iters, double *loss_v) {
    if (int rc = grid_check(h, g, false, "ev2g_grid_solve")) return rc;
    if (!p_kw || !q_kw || n_rows < 0) return fail(h, EV2G_ERR_ARG, "ev2g_grid_solve: p_kw or q_kw is null, or n_rows < 0");
    GridArgs ga{};
    ga.p = p_kw; ga.q = q_kw; ga.n_rows = n_rows; ga.vm = vm; ga.vc = v_complex; ga.iters = iters; ga.loss = loss_v;
    return grid_launch(h, g, ga, false);
}

// the grid kernel after the one-step launch of step h->current_step: a one-step launch leaves Transformer.current_power of its step in
// tr_power_now (every step kernel writes it in a launch's last step)
static int grid_launch_step(ev2g_handle *h, const ev2g_grid *g, double *vm, double *reward, double base_weight, double voltage_weight) {
    GridArgs ga{};
    ga.p = g->p_base; ga.q = g->q_base; ga.tr_power = h->st.tr_power_now; ga.M = h->M; ga.T1 = h->T + 1; ga.t = h->current_step;
    ga.scn_off = (int)h->scn_off; ga.n_rows = h->E; ga.vm = vm; ga.reward = reward;
    ga.base_weight = base_weight; ga.voltage_weight = voltage_weight;
    ga.vv_sum = g->vv_sum; ga.rew_sum = g->rew_sum; ga.vv_count = g->vv_count; ga.vv_steps = g->vv_steps;
    return grid_launch(h, g, ga, true);
}

// the state kernel for the handle's current step counter; a row written into the grid's own obs32 is remembered as valid for that counter
static int grid_launch_state(ev2g_handle *h, ev2g_grid *g, double *obs, float *obs32) {
    if (!obs && !obs32) return EV2G_OK;
    HeurArgs ha{};
    ha.port_slot = h->d_port_slot; ha.scn_off = (int)h->scn_off;
    const GridStateArgs sa{g->tf, g->tf_per_scn, g->p_base, g->q_base, g->n, h->current_step, g->Dg, obs, obs32};
    const long long total = (long long)h->E * g->Dg;
    const dim3 grid((unsigned)std::min<long long>((total + EV2G_GRID_STATE_BLOCK - 1) / EV2G_GRID_STATE_BLOCK, 1 << 20));
    hipLaunchKernelGGL(ev2g_grid_state_kernel, grid, dim3(EV2G_GRID_STATE_BLOCK), 0, h->stream, h->scn, h->st, ha, sa);
    HIPCHK(h, hipGetLastError());
    if (obs32 == g->obs32) { g->obs32_step = h->current_step; g->obs32_epoch = h->state_epoch; }
    return EV2G_OK;
}

static int grid_state_check(ev2g_handle *h, ev2g_grid *g, const char *who) {
    if (int rc = grid_check(h, g, true, who)) return rc;
    if (!g->tf) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no state attached to the grid (ev2g_grid_state_attach)");
    if (g->Dg != 6 + 2 * g->n + 3 * h->P) return fail(h, EV2G_ERR_ARG, std::string(who) + ": the loaded scenarios' ports differ from those the state was attached for");
    return EV2G_OK;
}

// ---- the runner of one-step launch chains (StepChain) ----
// k x ([agent | actor [-> widen] | actor-critic sample] [-> fail kernel | action wrapper] -> one-step launch [-> grid kernel] -> the step counter advances [-> delay kernel | float32
// copy] [-> state kernel of the next counter]).  Nothing but launches while no episode ends inside: ev2g_rollout captures it into a graph.
static int chain_steps(ev2g_handle *h, const StepChain &c, int k) {
    ev2g_link *l = c.link; ev2g_grid *g = c.grid;
    const long long adv = (c.auto_reset == EV2G_AUTO_RESET_NEXT) ? h->E % h->M : 0;   // pool offset advance per in-run reset
    const long long ED = (long long)h->E * h->D, EP = (long long)h->E * h->P;
    int rc;
    for (int i = 0; i < k; i++) {
        if (h->current_step >= h->T) {
            if (!c.auto_reset) return fail(h, EV2G_ERR_DONE, std::string(c.who) + ": episode finished before k_steps (auto_reset off)");
            if ((rc = ev2g_reset_ex(h, nullptr, h->scn_off + adv))) return rc;
        }
        const double *act_i = c.actions.at(i);   // what the step reads; null: the registered float32 actions
        if (c.agent && (rc = heuristic_launch(h, c.agent, c.actions.at(i)))) return rc;
        if (c.actor) {   // (it reads the object's OWN float32 row: an entry under an actor leaves obs / gobs32 to run_chain's defaults, which write it)
            const float *in32 = l ? l->obs32 : g ? g->obs32 : h->extras.obs_f32;
            float *out32 = l ? l->act32 : g ? g->act32 : (float *)h->extras.actions_f32;
            if ((rc = ev2g_mlp_forward(h, c.actor, in32, out32, h->E))) return rc;
            if (g) {
                const dim3 grid((unsigned)std::min<long long>((EP + EV2G_GRID_STATE_BLOCK - 1) / EV2G_GRID_STATE_BLOCK, 1 << 20));
                hipLaunchKernelGGL(ev2g_grid_widen_kernel, grid, dim3(EV2G_GRID_STATE_BLOCK), 0, h->stream, (const float *)g->act32, g->act, EP);
                HIPCHK(h, hipGetLastError());
                act_i = g->act;
            }
        }
        if (l && (c.actor || l->p_fail > 0.0)) {
            // (under an actor the fail kernel also widens the policy's float32 row into the float64 block the step reads: it runs for
            // p_fail = 0 too, where it holds nothing and draws no uniform)
            if ((rc = link_launch_act(h, l, h->current_step, c.actor ? (const void *)l->act32 : (const void *)act_i, c.actor != nullptr, nullptr))) return rc;
            act_i = l->held;
        }
        if (c.wrap) {
            double *out = c.wrapped.p ? c.wrapped.at(i) : c.wrap->act;
            if ((rc = wrap_launch(h, c.wrap, c.actor ? h->extras.actions_f32 : (const void *)act_i, c.actor != nullptr, out))) return rc;
            act_i = out;
        }
        if (c.ac) {
            if ((rc = ac_launch(h, c.ac, c.ac_obs.at(i), h->E, !c.ac_deterministic, nullptr, c.ac_actions.at(i), c.ac->clipped, c.ac_values.at(i),
                                c.ac_log_probs.at(i)))) return rc;
            if (!c.ac_direct)
                HIPCHK(h, hipMemcpyAsync((void *)h->extras.actions_f32, c.ac->clipped, EP * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        }
        if (c.ars) {
            if (c.ars_direct) {
                if ((rc = ars_launch(h, c.ars, c.ars->obs32, h->E, c.ars_population, c.ars->act32))) return rc;
            } else {
                if (i == 0) HIPCHK(h, hipMemcpyAsync(h->extras.obs_f32, c.ars->obs32, ED * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
                if ((rc = ars_launch(h, c.ars, (const float *)h->extras.obs_f32, h->E, c.ars_population, (float *)h->extras.actions_f32))) return rc;
            }
        }
        StepIO io = make_io(h, StepRows{{act_i, c.a_stride_to_kernel ? c.actions.stride : 0}, {c.obs.at(i)}, {c.reward.at(i)}, {c.done.at(i)}, {c.mask.at(i)}},
                            c.count_steps ? i : 0, 0);
        if (c.ac && c.ac_direct) { io.act32 = c.ac->clipped; io.obs32 = c.ac_obs.at(i + 1); }
        if (c.ars && c.ars_direct) { io.act32 = c.ars->act32; io.obs32 = c.ars->obs32; }
        if ((rc = launch_steps(h, io, h->current_step, 1, 0))) return rc;
        if (c.ars && !c.ars_direct)
            HIPCHK(h, hipMemcpyAsync(c.ars->obs32, h->extras.obs_f32, ED * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        if (c.ac && !c.ac_direct)
            HIPCHK(h, hipMemcpyAsync(c.ac_obs.at(i + 1), h->extras.obs_f32, ED * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        if (g && (rc = grid_launch_step(h, g, c.vm.at(i), c.reward.at(i), c.base_weight, c.voltage_weight))) return rc;
        h->current_step += 1;
        // (collect_direct promises the full instantiation; were it ever wrong the step has run and is counted, the rows of this step are not to be trusted)
        if (((c.ac && c.ac_direct) || (c.ars && c.ars_direct)) && h->last.specialisation <= 0) return fail(h, EV2G_ERR_STATE, std::string(c.who) + ": internal: the direct path needs the full instantiation");
        if (l && l->p_delay > 0.0) {
            if ((rc = link_launch_obs(h, l, h->current_step, c.obs.at(i), c.actor ? l->obs32 : nullptr))) return rc;
        } else if (l && c.actor) {
            const dim3 grid((unsigned)std::min<long long>((ED + EV2G_LINK_BLOCK - 1) / EV2G_LINK_BLOCK, 1 << 20));
            hipLaunchKernelGGL(ev2g_link_f32_kernel, grid, dim3(EV2G_LINK_BLOCK), 0, h->stream, (const double *)c.obs.at(i), l->obs32, ED);
            HIPCHK(h, hipGetLastError());
        }
        if (g && c.observed && (rc = grid_launch_state(h, g, c.gobs.at(i), c.gobs32.at(i)))) return rc;
    }
    return EV2G_OK;
}

// The timed call of a segment inside one episode: the checks every such entry makes (behind its own), the agent's, the link's and the grid's
// own blocks where the caller passes none, the bracket, the steps.
static int run_chain(ev2g_handle *h, StepChain c, int k) {
    const std::string who = c.who;
    ev2g_link *l = c.link; ev2g_grid *g = c.grid;
    if (k < 0 || c.actions.stride < 0 || c.obs.stride < 0 || c.reward.stride < 0 || c.done.stride < 0 || c.mask.stride < 0 || c.vm.stride < 0 ||
        c.gobs.stride < 0 || c.gobs32.stride < 0 || c.wrapped.stride < 0)
        return fail(h, EV2G_ERR_ARG, who + ": negative step count or stride");
    if (c.ac && (l || g || c.wrap))
        return fail(h, EV2G_ERR_ARG, who + ": a Gaussian actor-critic does not stack with a link, a grid or an action wrapper");
    if (c.ars && (l || g || c.wrap || c.ac || c.agent || c.actor))
        return fail(h, EV2G_ERR_ARG, who + ": an ARS learner does not stack with a link, a grid, an action wrapper or another action source");
    if (!c.agent && !c.actor && !c.ac && !c.ars && !c.actions.p) return fail(h, EV2G_ERR_ARG, who + ": without an agent the " + (l ? "raw " : "") + "actions are read from `actions`");
    // the engine resets lazily inside the step launch after an episode end, so an agent's launch for the new episode's first step would
    // read the finished episode's ports: segments stay inside one episode, the caller resets in between
    if (h->current_step + k > h->T) return fail(h, EV2G_ERR_DONE, who + ": the segment would run past the episode end");
    if (c.actor && g && !l && (g->obs32_step != h->current_step || g->obs32_epoch != h->state_epoch))
        return fail(h, EV2G_ERR_STATE, who + ": the grid's float32 row does not hold the state of step counter " + std::to_string(h->current_step) +
                                       " (ev2g_grid_observe first; a reset or a step outside the grid's calls invalidates it)");
    int rc;
    if (l) {   // (the link's blocks are allocated on first use)
        const size_t ED = (size_t)l->E * h->D, EP = (size_t)l->E * l->P;
        if (c.agent && !c.actions.p) { if ((rc = link_buffer(h, l, &l->raw, EP))) return rc; c.actions = {l->raw}; }
        if ((c.actor || l->p_delay > 0.0) && !c.obs.p) { if ((rc = link_buffer(h, l, &l->obs, ED))) return rc; c.obs = {l->obs}; }
        if (c.actor && ((rc = link_buffer(h, l, &l->obs32, ED)) || (rc = link_buffer(h, l, &l->act32, EP)))) return rc;
    }
    if (c.agent && !c.actions.p) c.actions = {c.agent->act};
    if (g) {
        if (!c.reward.p) c.reward = {g->rew};
        if (!c.vm.p) c.vm = {g->vm};
        if (c.observed && !c.gobs32.p) c.gobs32 = {g->obs32};   // the grid's own row stays the current counter's: ev2g_grid_rollout can go on from it
    }
    (void)hipSetDevice(h->device);
    if ((rc = timed_open(h)) || (rc = chain_steps(h, c, k))) return rc;
    return timed_close(h);
}

int ev2g_grid_run(ev2g_handle *h, ev2g_grid *g, ev2g_heuristic *a, int k_steps, double *actions, int64_t a_stride, double *obs, int64_t o_stride,
                  double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride, double *vm, int64_t v_stride,
                  double base_weight, double voltage_weight) {
    int rc = grid_check(h, g, true, "ev2g_grid_run");
    if (rc) return rc;
    if (a && (rc = heuristic_check(h, a, "ev2g_grid_run"))) return rc;
    StepChain c{"ev2g_grid_run"};
    c.agent = a; c.actions = {actions, a_stride};
    c.grid = g; c.base_weight = base_weight; c.voltage_weight = voltage_weight; c.vm = {vm, v_stride};
    c.obs = {obs, o_stride}; c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    return run_chain(h, c, k_steps);
}

int ev2g_grid_run_observed(ev2g_handle *h, ev2g_grid *g, ev2g_heuristic *a, int k_steps, double *actions, int64_t a_stride, double *obs,
                           int64_t o_stride, double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride,
                           double *vm, int64_t v_stride, double base_weight, double voltage_weight, double *gobs, int64_t go_stride, float *gobs32,
                           int64_t go32_stride) {
    int rc = grid_state_check(h, g, "ev2g_grid_run_observed");
    if (rc) return rc;
    if (a && (rc = heuristic_check(h, a, "ev2g_grid_run_observed"))) return rc;
    StepChain c{"ev2g_grid_run_observed"};
    c.agent = a; c.actions = {actions, a_stride};
    c.grid = g; c.base_weight = base_weight; c.voltage_weight = voltage_weight; c.vm = {vm, v_stride};
    c.observed = true; c.gobs = {gobs, go_stride}; c.gobs32 = {gobs32, go32_stride};
    c.obs = {obs, o_stride}; c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    return run_chain(h, c, k_steps);
}

int ev2g_grid_state_attach(ev2g_handle *h, ev2g_grid *g, const double *time_features, int per_scenario) {
    if (int rc = grid_check(h, g, true, "ev2g_grid_state_attach")) return rc;
    if (!time_features) return fail(h, EV2G_ERR_ARG, "ev2g_grid_state_attach: time_features is null");
    const int Dg = 6 + 2 * g->n + 3 * h->P;
    const size_t ED = (size_t)h->E * Dg, EP = (size_t)h->E * h->P, tfn = (size_t)(per_scenario ? h->M : 1) * (h->T + 1) * 3;
    const auto detach = [g] {
        free_pool(g->swap_allocs);
        g->tf = g->obs = g->act = nullptr; g->obs32 = g->act32 = nullptr;
        g->Dg = 0; g->obs32_step = -1; g->obs32_epoch = -1;
    };
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (a second attach replaces blocks that queued kernels may still read)
    detach();
    int rc = upload(h, g->swap_allocs, time_features, tfn, &g->tf);
    if (!rc) rc = dalloc(h, g->swap_allocs, ED, &g->obs);
    if (!rc) rc = dalloc(h, g->swap_allocs, ED, &g->obs32);
    if (!rc) rc = dalloc(h, g->swap_allocs, EP, &g->act);
    if (!rc) rc = dalloc(h, g->swap_allocs, EP, &g->act32);
    const int drained = drain(h);   // (time_features is the caller's: also behind a failure)
    if (!rc) rc = drained;
    if (rc) {
        detach();
        return rc;
    }
    g->tf_per_scn = per_scenario ? 1 : 0;
    g->Dg = Dg;
    return EV2G_OK;
}

int ev2g_grid_state_dim(ev2g_handle *h, ev2g_grid *g) {
    if (!h || !g || std::find(h->grids.begin(), h->grids.end(), g) == h->grids.end() || !g->tf) return -1;
    return g->Dg;
}

int ev2g_grid_observe(ev2g_handle *h, ev2g_grid *g, double *obs, float *obs32) {
    if (int rc = grid_state_check(h, g, "ev2g_grid_observe")) return rc;
    // the caller's blocks, and the grid's own rows (what ev2g_grid_rollout's first forward pass reads)
    if (int rc = grid_launch_state(h, g, obs, obs32)) return rc;
    return grid_launch_state(h, g, g->obs, g->obs32);
}

int ev2g_grid_rollout(ev2g_handle *h, ev2g_grid *g, const ev2g_mlp *m, int k_steps, double *reward, int64_t r_stride, uint8_t *done,
                      int64_t d_stride, uint8_t *mask, int64_t m_stride, double *vm, int64_t v_stride, double base_weight, double voltage_weight) {
    int rc = grid_state_check(h, g, "ev2g_grid_rollout");
    if (rc) return rc;
    if (!m || k_steps < 0 || r_stride < 0 || d_stride < 0 || m_stride < 0 || v_stride < 0) return fail(h, EV2G_ERR_ARG, "ev2g_grid_rollout: bad arguments");
    if (m->dev.d_in != g->Dg || m->dev.d_out != h->P) return fail(h, EV2G_ERR_ARG, "ev2g_grid_rollout: actor shape != (grid state dim, ports)");
    StepChain c{"ev2g_grid_rollout"};
    c.actor = m;
    c.grid = g; c.base_weight = base_weight; c.voltage_weight = voltage_weight; c.vm = {vm, v_stride};
    c.observed = true;   // (into the grid's own float32 row: the next forward pass reads it)
    c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    return run_chain(h, c, k_steps);
}

int ev2g_grid_get_stats(ev2g_handle *h, ev2g_grid *g, double *vv_sum, int32_t *vv_count, int32_t *vv_steps, double *rew_sum) {
    if (int rc = grid_check(h, g, true, "ev2g_grid_get_stats")) return rc;
    const size_t Ed = (size_t)h->E * sizeof(double), Ei = (size_t)h->E * sizeof(int32_t);
    if (vv_sum) HIPCHK(h, hipMemcpyAsync(vv_sum, g->vv_sum, Ed, hipMemcpyDeviceToHost, h->stream));
    if (vv_count) HIPCHK(h, hipMemcpyAsync(vv_count, g->vv_count, Ei, hipMemcpyDeviceToHost, h->stream));
    if (vv_steps) HIPCHK(h, hipMemcpyAsync(vv_steps, g->vv_steps, Ei, hipMemcpyDeviceToHost, h->stream));
    if (rew_sum) HIPCHK(h, hipMemcpyAsync(rew_sum, g->rew_sum, Ed, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

const char *ev2g_last_launch_timing(const ev2g_handle *h) { return h ? timing_kind_name(h->ring.last_kind()) : ""; }

double ev2g_last_step_n_kernel_ms(ev2g_handle *h) {
    return ev2g_step_n_kernel_ms_back(h, 0);
}

double ev2g_step_n_kernel_ms_back(ev2g_handle *h, int back) {
    if (!h) return -1.0;
    const int slot = h->ring.slot_of(back);
    if (slot < 0) return -1.0;
    if (h->ring.kind[slot] == TIMING_STAMPS) {   // the kernel's own stamps: behind everything queued on the stream, the slot's two words
        unsigned long long w[2] = {0, 0};
        (void)hipSetDevice(h->device);
        if (hipStreamSynchronize(h->stream) != hipSuccess) return -1.0;
        if (hipMemcpy(w, h->d_stamps + 2 * (size_t)slot, sizeof w, hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
        return timing_stamp_ms(w[0], w[1], h->wall_khz);
    }
    if (hipEventSynchronize(h->ev1s[slot]) != hipSuccess) return -1.0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev0s[slot], h->ev1s[slot]) != hipSuccess) return -1.0;
    return (double)ms;
}

// ---- action wrappers (ev2g_wrap.h) ----
// what a wrapper kind needs of the loaded scenarios beyond their envs and ports; asked at create and again before every launch, as for the agents
static int wrap_shape_check(ev2g_handle *h, int kind, const std::string &who) {
    if (kind != EV2G_WRAP_RESCALE_REPAIR) return EV2G_OK;
    // the reference asserts it (action_wrappers.py:186) and indexes its per-charger tables with port ids and queue positions
    if (h->P != h->C)
        return fail(h, EV2G_ERR_ARG, who + ": Rescale_RepairLayer needs one port per charger (action_wrappers.py:186)");
    // one env's queue stage has to fit the 64 KiB of LDS
    if (h->P > EV2G_WRAP_MAX_PORTS || ev2g_wrap_wave_bytes(h->P) > 65536)
        return fail(h, EV2G_ERR_ARG, who + ": Rescale_RepairLayer supports up to " + std::to_string(EV2G_WRAP_MAX_PORTS) + " ports per env");
    return EV2G_OK;
}

// the device stage of a wrapper: its float64 block and, for the repair layer, the queue with its power lists
static int wrap_device_stage(ev2g_handle *h, ev2g_wrap *w) {
    if (int rc = dalloc(h, w->allocs, (size_t)w->E * w->P, &w->act)) return rc;
    return w->kind == EV2G_WRAP_RESCALE_REPAIR ? queue_alloc(h, w->allocs, w->E, w->P, true, &w->q) : EV2G_OK;
}

int ev2g_wrap_create(ev2g_handle *h, int kind, ev2g_wrap **out) {
    if (!h || !out) return fail(h, EV2G_ERR_ARG, "ev2g_wrap_create: null argument");
    *out = nullptr;
    if (!h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_wrap_create: no scenarios loaded");
    if (kind < EV2G_WRAP_BINARY || kind > EV2G_WRAP_RESCALE_REPAIR) return fail(h, EV2G_ERR_ARG, "ev2g_wrap_create: unknown wrapper kind");
    if (int rc = wrap_shape_check(h, kind, "ev2g_wrap_create")) return rc;
    (void)hipSetDevice(h->device);
    ev2g_wrap *w = new ev2g_wrap();
    w->kind = kind; w->E = h->E; w->P = h->P;
    return owned_created(h, &ev2g_handle::wraps, w, wrap_device_stage(h, w), out);
}

void ev2g_wrap_destroy(ev2g_handle *h, ev2g_wrap *w) { owned_destroy(h, &ev2g_handle::wraps, w); }

static int wrap_check(ev2g_handle *h, ev2g_wrap *w, const char *who) {
    if (int rc = owned_check(h, &ev2g_handle::wraps, w, "wrapper", who)) return rc;
    if (w->E != h->E || w->P != h->P)
        return fail(h, EV2G_ERR_ARG, std::string(who) + ": the loaded scenarios' envs / ports differ from those the wrapper was created for");
    return wrap_shape_check(h, w->kind, who);
}

int ev2g_wrap_reset_state(ev2g_handle *h, ev2g_wrap *w) {
    if (int rc = wrap_check(h, w, "ev2g_wrap_reset_state")) return rc;
    if (w->q.qlen) HIPCHK(h, hipMemsetAsync(w->q.qlen, 0, (size_t)w->E * sizeof(int), h->stream));
    return EV2G_OK;
}

// the wrapper's actions for the current step: in [E, P] (float64, or float32 with in32) -> out [E, P] float64 (may be a float64 `in`); the
// repair layer's queue advances
static int wrap_launch(ev2g_handle *h, ev2g_wrap *w, const void *in, bool in32, double *out) {
    const DevScn &s = h->scn;
    if (w->kind == EV2G_WRAP_RESCALE_REPAIR) {
        // one wavefront per env, up to four per workgroup while their LDS stages fit 64 KiB
        const WrapArgs wa{h->d_port_slot, h->d_heur_cs_kw, h->d_heur_cs_min_kw, w->q.queue, w->q.qlen, w->q.qmin, w->q.qmax, (int)h->scn_off};
        const size_t wb = ev2g_wrap_wave_bytes(s.P);   // (<= 64 KiB: wrap_shape_check)
        const int epb = (int)std::min<size_t>(EV2G_WRAP_BLOCK / 64, 65536 / wb);
        const dim3 grid((s.E + epb - 1) / epb), block(64 * epb);
        const int t = h->current_step;
        if (in32) hipLaunchKernelGGL(ev2g_wrap_repair_kernel<true>, grid, block, epb * wb, h->stream, s, h->st, wa, t, in, out);
        else hipLaunchKernelGGL(ev2g_wrap_repair_kernel<false>, grid, block, epb * wb, h->stream, s, h->st, wa, t, in, out);
    } else {
        const long long n = (long long)s.E * s.P;
        const dim3 grid((unsigned)std::min<long long>((n + EV2G_WRAP_BLOCK - 1) / EV2G_WRAP_BLOCK, 1 << 20));
        const int kind = w->kind == EV2G_WRAP_BINARY ? EV2G_WRAP_KIND_BINARY : EV2G_WRAP_KIND_THREE_STEP;
        if (in32) hipLaunchKernelGGL(ev2g_wrap_discrete_kernel<true>, grid, dim3(EV2G_WRAP_BLOCK), 0, h->stream, s, (const int *)h->d_port_slot, kind, in, out);
        else hipLaunchKernelGGL(ev2g_wrap_discrete_kernel<false>, grid, dim3(EV2G_WRAP_BLOCK), 0, h->stream, s, (const int *)h->d_port_slot, kind, in, out);
    }
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_wrap_actions(ev2g_handle *h, ev2g_wrap *w, const void *in, int in_is_f32, double *out) {
    if (int rc = wrap_check(h, w, "ev2g_wrap_actions")) return rc;
    if (!in || !out) return fail(h, EV2G_ERR_ARG, "ev2g_wrap_actions: the action block is null");
    if (h->current_step >= h->T) return fail(h, EV2G_ERR_DONE, "ev2g_wrap_actions: episode is done, reset the environment");
    return wrap_launch(h, w, in, in_is_f32 != 0, out);
}

int ev2g_wrap_run(ev2g_handle *h, ev2g_wrap *w, int k_steps, double *actions, int64_t a_stride, double *wrapped, int64_t w_stride, double *obs,
                  int64_t o_stride, double *reward, int64_t r_stride, uint8_t *done, int64_t d_stride, uint8_t *mask, int64_t m_stride) {
    if (int rc = wrap_check(h, w, "ev2g_wrap_run")) return rc;
    StepChain c{"ev2g_wrap_run"};
    c.actions = {actions, a_stride};
    c.wrap = w; c.wrapped = {wrapped, w_stride};
    c.obs = {obs, o_stride}; c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    return run_chain(h, c, k_steps);
}

int ev2g_wrap_rollout(ev2g_handle *h, ev2g_wrap *w, const ev2g_mlp *m, int k_steps, double *reward, int64_t r_stride, uint8_t *done,
                      int64_t d_stride, uint8_t *mask, int64_t m_stride) {
    if (int rc = wrap_check(h, w, "ev2g_wrap_rollout")) return rc;
    if (!m || k_steps < 0 || r_stride < 0 || d_stride < 0 || m_stride < 0) return fail(h, EV2G_ERR_ARG, "ev2g_wrap_rollout: bad arguments");
    if (w->kind == EV2G_WRAP_THREE_STEP)
        return fail(h, EV2G_ERR_ARG, "ev2g_wrap_rollout: ThreeStep_Action takes the discrete actions 0 / 1 / 2, which an actor's tanh output never equals");
    const ev2g_step_extras &x = h->extras;
    if (!x.obs_f32 || !x.actions_f32 || x.obs_f32_step_stride != 0)
        return fail(h, EV2G_ERR_ARG, "ev2g_wrap_rollout: register float32 observation (step stride 0) and action buffers with ev2g_set_step_extras first");
    if (m->dev.d_in != h->D || m->dev.d_out != h->P) return fail(h, EV2G_ERR_ARG, "ev2g_wrap_rollout: actor shape != (obs dim, ports)");
    // the unfused policy loop between the registered float32 pair, the wrapper between actor and step: no fused variant, no graph capture
    StepChain c{"ev2g_wrap_rollout"};
    c.actor = m;
    c.wrap = w;
    c.reward = {reward, r_stride}; c.done = {done, d_stride}; c.mask = {mask, m_stride};
    c.count_steps = x.cost != nullptr;   // (as ev2g_rollout: a cost buffer may record every step; the float32 buffers do not advance)
    return run_chain(h, c, k_steps);
}

// ---- the Gaussian actor-critic and GAE (ev2g_ac.h) ----
// AcDev's twelve image pointers under their AcSlot: the order of ac_array_sizes / pack_ac (ev2g_policy_host.h)
static std::array<const float **, AC_ARRAYS> ac_arrays(AcDev &d) {
    return {&d.w1, &d.b1, &d.w2, &d.b2, &d.w3, &d.b3, &d.u1, &d.c1, &d.u2, &d.c2, &d.u3, &d.c3};
}

// (a policy's entries run without scenarios, ev2g_ac_collect apart)
static int ac_check(ev2g_handle *h, ev2g_acpolicy *ac, const char *who) { return owned_check(h, &ev2g_handle::acs, ac, "actor-critic", who, false); }

// packs the twelve host arrays into the object's device arrays (allocated at create) and drains the stream: the staging vectors are temporaries
static int ac_upload_weights(ev2g_handle *h, ev2g_acpolicy *ac, const AcWeights &w) {
    const auto stage = pack_ac(ac->plan, w);
    const auto dst = ac_arrays(ac->dev);
    for (int i = 0; i < AC_ARRAYS; i++)
        HIPCHK(h, hipMemcpyAsync((void *)*dst[i], stage[i].data(), stage[i].size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

static int ac_upload_log_std(ev2g_handle *h, ev2g_acpolicy *ac, const float *log_std, const char *who) {
    const int P = ac->dev.d_out;
    std::vector<float> sigma((size_t)P);
    std::vector<double> a((size_t)P), c((size_t)P);
    for (int p = 0; p < P; p++) {
        if (!std::isfinite(log_std[p])) return fail(h, EV2G_ERR_ARG, std::string(who) + ": log_std[" + std::to_string(p) + "] is not finite");
        const double s = std::exp((double)log_std[p]);
        sigma[p] = (float)s;
        const double sf = (double)sigma[p];   // (the float32 sigma the sample is scaled by)
        a[p] = 1.0 / (2.0 * sf * sf);
        c[p] = -(double)log_std[p] - 0.9189385332046727;   // log(2 pi) / 2
    }
    HIPCHK(h, hipMemcpyAsync((void *)ac->dev.sigma, sigma.data(), P * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync((void *)ac->dev.lp_a, a.data(), P * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync((void *)ac->dev.lp_c, c.data(), P * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ac->log_std.assign(log_std, log_std + P);
    return EV2G_OK;
}

static void ppo_launch_repack(ev2g_handle *h, ev2g_ppo *p, bool transposed_only) {
    hipLaunchKernelGGL(ev2g_ppo_repack_kernel, dim3((unsigned)p->n_blocks), dim3(256), 0, h->stream, p->map, (const float *)p->theta, transposed_only ? 1 : 0);
}

// a bound learner's masters (and its transposed images) follow ev2g_ac_set_weights / ev2g_ac_set_log_std; Adam's state is kept
static int ppo_reset_masters(ev2g_handle *h, ev2g_ppo *p, const AcWeights *w, const float *log_std) {
    const PpoPlan &pl = p->plan;
    auto master = [&](int i, const float *src) {
        return hipMemcpyAsync(p->theta + pl.off[i], src, (size_t)(pl.off[i + 1] - pl.off[i]) * sizeof(float), hipMemcpyHostToDevice, h->stream);
    };
    if (w) {
        for (int i = 0; i < AC_ARRAYS; i++) HIPCHK(h, master(i, w->a[i]));
        ppo_launch_repack(h, p, true);
        HIPCHK(h, hipGetLastError());
    }
    if (log_std) HIPCHK(h, master(AC_ARRAYS, log_std));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the sources are the caller's
    return EV2G_OK;
}

static bool ac_weights_null(const AcWeights &w) {
    for (const float *a : w.a)
        if (!a) return true;
    return false;
}

// the device stage of an actor-critic: allocates the twelve images and the log_std arrays, uploads them and sets the kernel's dynamic-LDS attribute
static int ac_device_stage(ev2g_handle *h, ev2g_acpolicy *ac, const AcWeights &w, const float *log_std) {
    AcDev &d = ac->dev;
    const auto sizes = ac_array_sizes(ac->plan);
    const auto arrays = ac_arrays(d);
    for (size_t i = 0; i < AC_ARRAYS; i++)
        if (int rc = dalloc(h, ac->allocs, sizes[i], arrays[i])) return rc;
    if (int rc = dalloc(h, ac->allocs, (size_t)d.d_out, &d.sigma)) return rc;
    for (const double **dst : {&d.lp_a, &d.lp_c})
        if (int rc = dalloc(h, ac->allocs, (size_t)d.d_out, dst)) return rc;
    if (int rc = ac_upload_weights(h, ac, w)) return rc;
    if (int rc = ac_upload_log_std(h, ac, log_std, "ev2g_ac_create")) return rc;
    if (ac->lds > 48 * 1024 && !(h->ac_attr_mask & (1u << ac->relu))) {   // (function attributes are per device: once per handle)
        const hipError_t e = hipFuncSetAttribute(ac_kernel(ac->relu).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ev2g_ac_lds_max());
        if (e != hipSuccess) return fail(h, EV2G_ERR_HIP, std::string("ev2g_ac_create: hipFuncSetAttribute: ") + hipGetErrorString(e));
        h->ac_attr_mask |= 1u << ac->relu;
    }
    return EV2G_OK;
}

int ev2g_ac_create(ev2g_handle *h, int d_in, int h1, int h2, int v1, int v2, int d_out, int activation, const float *pi_W1, const float *pi_b1,
                   const float *pi_W2, const float *pi_b2, const float *vf_W1, const float *vf_b1, const float *vf_W2, const float *vf_b2,
                   const float *action_W, const float *action_b, const float *value_W, const float *value_b, const float *log_std, float lo,
                   uint64_t seed, ev2g_acpolicy **out) {
    if (!h || !out) return fail(h, EV2G_ERR_ARG, "ev2g_ac_create: null argument");
    *out = nullptr;
    const AcWeights w{{pi_W1, pi_b1, pi_W2, pi_b2, vf_W1, vf_b1, vf_W2, vf_b2, action_W, action_b, value_W, value_b}};
    if (ac_weights_null(w) || !log_std) return fail(h, EV2G_ERR_ARG, "ev2g_ac_create: a weight, bias or log_std pointer is null");
    const AcPlan p = plan_ac(d_in, h1, h2, v1, v2, d_out);
    if (p.err) return fail(h, p.err, p.refusal);
    if (activation != EV2G_AC_TANH && activation != EV2G_AC_RELU) return fail(h, EV2G_ERR_ARG, "ev2g_ac_create: activation must be EV2G_AC_TANH or EV2G_AC_RELU");
    if (lo != -1.0f && lo != 0.0f) return fail(h, EV2G_ERR_ARG, "ev2g_ac_create: lo must be -1 or 0");
    for (int i = 0; i < d_out; i++)
        if (!std::isfinite(log_std[i])) return fail(h, EV2G_ERR_ARG, "ev2g_ac_create: log_std[" + std::to_string(i) + "] is not finite");
    (void)hipSetDevice(h->device);
    ev2g_acpolicy *ac = new ev2g_acpolicy();
    ac->plan = p;
    AcDev &d = ac->dev;
    d.d_in = d_in; d.h1 = h1; d.h2 = h2; d.v1 = v1; d.v2 = v2; d.d_out = d_out;
    d.k1 = p.k1; d.n1 = p.n1; d.n2 = p.n2; d.m1 = p.m1; d.m2 = p.m2; d.n3 = p.n3;
    d.lo = lo;
    ac->relu = activation == EV2G_AC_RELU;
    ac->seed = seed; ac->n = 0;
    ac->lds = ev2g_ac_lds(d).bytes;
    return owned_created(h, &ev2g_handle::acs, ac, ac_device_stage(h, ac, w, log_std), out);
}

// (a bound learner goes with its policy)
void ev2g_ac_destroy(ev2g_handle *h, ev2g_acpolicy *ac) {
    if (h && ac && std::find(h->acs.begin(), h->acs.end(), ac) != h->acs.end() && ac->learner) owned_destroy(h, &ev2g_handle::ppos, ac->learner, ppo_free);
    owned_destroy(h, &ev2g_handle::acs, ac);
}

int ev2g_ac_seed(ev2g_handle *h, ev2g_acpolicy *ac, uint64_t seed, uint64_t first_draw) {
    if (int rc = ac_check(h, ac, "ev2g_ac_seed")) return rc;
    ac->seed = seed; ac->n = first_draw;
    return EV2G_OK;
}

int ev2g_ac_set_log_std(ev2g_handle *h, ev2g_acpolicy *ac, const float *log_std) {
    if (int rc = ac_check(h, ac, "ev2g_ac_set_log_std")) return rc;
    if (!log_std) return fail(h, EV2G_ERR_ARG, "ev2g_ac_set_log_std: log_std is null");
    for (int p = 0; p < ac->dev.d_out; p++)   // (checked before anything is enqueued: a refused call leaves the object as it was)
        if (!std::isfinite(log_std[p])) return fail(h, EV2G_ERR_ARG, "ev2g_ac_set_log_std: log_std[" + std::to_string(p) + "] is not finite");
    HIPCHK(h, hipStreamSynchronize(h->stream));   // launches still reading the old values
    if (int rc = ac_upload_log_std(h, ac, log_std, "ev2g_ac_set_log_std")) return rc;
    return ac->learner ? ppo_reset_masters(h, ac->learner, nullptr, log_std) : EV2G_OK;
}

int ev2g_ac_set_weights(ev2g_handle *h, ev2g_acpolicy *ac, const float *pi_W1, const float *pi_b1, const float *pi_W2, const float *pi_b2,
                        const float *vf_W1, const float *vf_b1, const float *vf_W2, const float *vf_b2, const float *action_W,
                        const float *action_b, const float *value_W, const float *value_b) {
    if (int rc = ac_check(h, ac, "ev2g_ac_set_weights")) return rc;
    const AcWeights w{{pi_W1, pi_b1, pi_W2, pi_b2, vf_W1, vf_b1, vf_W2, vf_b2, action_W, action_b, value_W, value_b}};
    if (ac_weights_null(w)) return fail(h, EV2G_ERR_ARG, "ev2g_ac_set_weights: a weight or bias pointer is null");
    if (int rc = ac_upload_weights(h, ac, w)) return rc;   // (stream-ordered behind the launches that read the old weights)
    return ac->learner ? ppo_reset_masters(h, ac->learner, &w, nullptr) : EV2G_OK;
}

// one launch of ev2g_ac_act_kernel over n_rows rows; a sampling launch takes the object's counter and advances it
static int ac_launch(ev2g_handle *h, ev2g_acpolicy *ac, const float *x, int n_rows, bool sample, float *mean, float *actions, float *clipped,
                     float *value, float *log_prob) {
    const LaunchDims dims{dim3((unsigned)((n_rows + EV2G_AC_ROWS - 1) / EV2G_AC_ROWS)), ac->lds, h->stream};
    ac_kernel(ac->relu).launch(dims, ac->dev, x, n_rows, sample ? 1 : 0, (uint64_t)ac->seed, (uint64_t)ac->n * (uint64_t)n_rows, mean, actions, clipped, value,
                               log_prob);
    HIPCHK(h, hipGetLastError());
    if (sample) ac->n += 1;
    return EV2G_OK;
}

int ev2g_ac_forward(ev2g_handle *h, ev2g_acpolicy *ac, const float *obs32, int n_rows, float *mean, float *value) {
    if (int rc = ac_check(h, ac, "ev2g_ac_forward")) return rc;
    if (!obs32 || n_rows <= 0) return fail(h, EV2G_ERR_ARG, "ev2g_ac_forward: obs32 is null or n_rows is not positive");
    return ac_launch(h, ac, obs32, n_rows, false, mean, nullptr, nullptr, value, nullptr);
}

int ev2g_ac_act(ev2g_handle *h, ev2g_acpolicy *ac, const float *obs32, int n_rows, int deterministic, float *actions, float *clipped, float *value,
                float *log_prob) {
    if (int rc = ac_check(h, ac, "ev2g_ac_act")) return rc;
    if (!obs32 || n_rows <= 0) return fail(h, EV2G_ERR_ARG, "ev2g_ac_act: obs32 is null or n_rows is not positive");
    return ac_launch(h, ac, obs32, n_rows, !deterministic, nullptr, actions, clipped, value, log_prob);
}

int ev2g_ac_collect(ev2g_handle *h, ev2g_acpolicy *ac, int k_steps, int deterministic, const ev2g_onpolicy_rows *r) {
    if (int rc = ac_check(h, ac, "ev2g_ac_collect")) return rc;
    if (!h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_ac_collect: no scenarios loaded");
    if (!r || k_steps < 0 || !r->obs || !r->actions || !r->values || !r->log_probs || !r->reward || !r->done || !r->mask)
        return fail(h, EV2G_ERR_ARG, "ev2g_ac_collect: null argument (every row array is required)");
    if (ac->dev.d_in != h->D) return fail(h, EV2G_ERR_ARG, "ev2g_ac_collect: d_in " + std::to_string(ac->dev.d_in) + " != the observation width " + std::to_string(h->D));
    if (ac->dev.d_out != h->P) return fail(h, EV2G_ERR_ARG, "ev2g_ac_collect: d_out " + std::to_string(ac->dev.d_out) + " != the ports " + std::to_string(h->P));
    const size_t ED = (size_t)h->E * h->D, EP = (size_t)h->E * h->P;
    const ev2g_step_extras &x = h->extras;
    const bool direct = collect_direct(h);   // the two routes of ev2g_collect's unfused loop
    if (!direct && !(x.obs_f32 && x.actions_f32 && x.obs_f32_step_stride == 0))
        return fail(h, EV2G_ERR_ARG, "ev2g_ac_collect: this configuration steps through the registered float32 hand-over buffers: register them with "
                                     "ev2g_set_step_extras (observation step stride 0) first");
    if (ac->clipped_elems < EP) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        free_pool(ac->swap_allocs); ac->clipped = nullptr; ac->clipped_elems = 0;
        if (int rc = dalloc(h, ac->swap_allocs, EP, &ac->clipped)) return rc;
        ac->clipped_elems = EP;
    }
    StepChain c{"ev2g_ac_collect"};
    c.ac = ac; c.ac_deterministic = deterministic != 0; c.ac_direct = direct;
    c.ac_obs = {r->obs, (long long)ED}; c.ac_actions = {r->actions, (long long)EP}; c.ac_values = {r->values, h->E}; c.ac_log_probs = {r->log_probs, h->E};
    c.reward = {r->reward, h->E}; c.done = {r->done, h->E}; c.mask = {r->mask, (long long)EP};
    c.count_steps = false;   // (as ev2g_collect: the registered buffers do not advance)
    return run_chain(h, c, k_steps);
}

void ev2g_ac_host_normal(float *dst, int64_t n_values, uint64_t seed, uint64_t first_index) {
    for (int64_t i = 0; i < n_values; i++) dst[i] = ev2g_ac_normal(seed, first_index + (uint64_t)i);
}

static int gae_args(ev2g_handle *h, const char *who, const void *a, const void *b, const void *c, const void *d, const void *e, const void *f,
                    const void *g, int k, int n_envs) {
    if (!a || !b || !c || !d || !e || !f || !g) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (k < 1 || n_envs < 1) return fail(h, EV2G_ERR_ARG, std::string(who) + ": k and n_envs must be positive");
    return EV2G_OK;
}

int ev2g_gae(ev2g_handle *h, const double *reward, const float *values, const uint8_t *episode_starts, const float *last_values,
             const uint8_t *last_dones, int k, int n_envs, double gamma, double lambda, float *advantages, float *returns) {
    if (!h) return fail(h, EV2G_ERR_ARG, "ev2g_gae: null handle");
    if (int rc = gae_args(h, "ev2g_gae", reward, values, episode_starts, last_values, last_dones, advantages, returns, k, n_envs)) return rc;
    (void)hipSetDevice(h->device);
    hipLaunchKernelGGL(ev2g_gae_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, h->stream, reward, values, episode_starts, last_values, last_dones, k,
                       n_envs, (float)gamma, (float)(gamma * lambda), advantages, returns);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_host_gae(const double *reward, const float *values, const uint8_t *episode_starts, const float *last_values, const uint8_t *last_dones,
                  int k, int n_envs, double gamma, double lambda, float *advantages, float *returns) {
    if (int rc = gae_args(nullptr, "ev2g_host_gae", reward, values, episode_starts, last_values, last_dones, advantages, returns, k, n_envs)) return rc;
    const float g = (float)gamma, c = (float)(gamma * lambda);
    for (int e = 0; e < n_envs; e++) ev2g_gae_env(reward, values, episode_starts, last_values, last_dones, k, n_envs, e, g, c, advantages, returns);
    return EV2G_OK;
}

// ---- the learners (ev2g_ppo.h): PPO and A2C ----
static int ppo_check(ev2g_handle *h, ev2g_ppo *p, const char *who) { return owned_check(h, &ev2g_handle::ppos, p, "learner", who, false); }

// an entry that drives one kind of learner on the other kind
static int learner_check(ev2g_handle *h, ev2g_ppo *p, const char *who, int kind) {
    if (int rc = ppo_check(h, p, who)) return rc;
    if (p->spec.kind != kind)
        return fail(h, EV2G_ERR_STATE, std::string(who) + (p->spec.kind == LEARNER_A2C    ? ": the learner is an A2C learner (the ev2g_a2c_* entries drive it)"
                                                           : p->spec.kind == LEARNER_TRPO ? ": the learner is a TRPO learner (the ev2g_trpo_* entries drive it)"
                                                                                          : ": the learner is a PPO learner (the ev2g_ppo_* entries drive it)"));
    return EV2G_OK;
}

int ev2g_ppo_query(int d_in, int h1, int h2, int v1, int v2, int d_out, ev2g_ppo_info *info) {
    if (!info) return fail(nullptr, EV2G_ERR_ARG, "ev2g_ppo_query: info is null");
    const PpoPlan p = plan_ppo(d_in, h1, h2, v1, v2, d_out);
    if (p.err) return fail(nullptr, p.err, p.refusal);
    info->lds_bytes = (int64_t)p.lds.bytes; info->workspace_bytes = (int64_t)p.workspace_bytes;
    info->grid_cap = p.grid_cap; info->n_params = p.n_params;
    return EV2G_OK;
}

// a config's fields, or the ones a set-rate entry sets, against their rules (ev2g_learner_host.h)
static int fields_check(ev2g_handle *h, const char *who, const std::vector<LearnerField> &fields) {
    const std::string refusal = learner_refusal(who, fields);
    return refusal.empty() ? EV2G_OK : fail(h, EV2G_ERR_ARG, refusal);
}

// the twelve arrays of a policy in SB3's layout from its packed images (out[i]: host pointers in the table's order)
static int ac_read_images(ev2g_handle *h, ev2g_acpolicy *ac, float *const out[AC_ARRAYS]) {
    const auto sizes = ac_array_sizes(ac->plan);
    const auto src = ac_arrays(ac->dev);
    std::array<std::vector<float>, AC_ARRAYS> stage;
    for (size_t i = 0; i < AC_ARRAYS; i++) {
        stage[i].resize(sizes[i]);
        HIPCHK(h, hipMemcpyAsync(stage[i].data(), *src[i], sizes[i] * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unpack_ac(ac->plan, stage, out);
    return EV2G_OK;
}

// the device stage of a learner: allocates its buffers, takes the masters from the policy's images, builds the map the kernels place elements by,
// fills the transposed images and sets the gradient kernel's dynamic-LDS attribute
static int ppo_device_stage(ev2g_handle *h, ev2g_ppo *p, ev2g_acpolicy *ac, const char *who) {
    const PpoPlan &pl = p->plan;
    const size_t G = (size_t)pl.n_params;
    const struct { float **dst; size_t n; } f32[] = {{&p->theta, G}, {&p->m, G}, {&p->v, G}, {&p->grad, G}, {&p->work, (size_t)pl.grid_cap * pl.slab_floats}};
    const struct { double **dst; size_t n; } f64[] = {{&p->stat_part, (size_t)pl.grid_cap * 8}, {&p->norm_part, (size_t)p->n_blocks}, {&p->advstat, 2}};
    for (const auto &b : f32)
        if (int rc = dalloc(h, p->allocs, b.n, b.dst)) return rc;
    for (const auto &b : f64)
        if (int rc = dalloc(h, p->allocs, b.n, b.dst)) return rc;
    float *img_t[3] = {nullptr, nullptr, nullptr};
    for (const AcParam &a : ac_params(pl.ac))
        if (a.slot_t != AC_NO_IMAGE_T)
            if (int rc = dalloc(h, p->allocs, a.img_floats, &img_t[a.slot_t])) return rc;
    // the masters: the policy's current numbers, read back from its images (exact: the images hold the float32 values themselves)
    std::vector<float> host(G, 0.f);
    float *dst[AC_ARRAYS];
    for (int i = 0; i < AC_ARRAYS; i++) dst[i] = host.data() + pl.off[i];
    if (int rc = ac_read_images(h, ac, dst)) return rc;
    std::copy(ac->log_std.begin(), ac->log_std.end(), host.begin() + pl.off[AC_ARRAYS]);
    PpoDev &d = p->dev;
    d.k1r = pl.k1r; d.w2t = img_t[AC_W2T]; d.w3t = img_t[AC_W3T]; d.u2t = img_t[AC_U2T]; d.log_std = p->theta + pl.off[AC_ARRAYS];
    std::copy(pl.slab_off, pl.slab_off + EV2G_PPO_ARRAYS, d.slab_off);
    d.slab_floats = pl.slab_floats;
    float *img[AC_ARRAYS];
    const auto arrays = ac_arrays(ac->dev);
    for (size_t i = 0; i < AC_ARRAYS; i++) img[i] = (float *)*arrays[i];
    p->map = ppo_map(pl, img, img_t);
    hipError_t e = hipMemcpyAsync(p->theta, host.data(), G * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) { ppo_launch_repack(h, p, true); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    const int relu = ac->relu ? 1 : 0, head = p->spec.head;
    const unsigned bit = 1u << (relu + 2 * head);
    if (e == hipSuccess && p->spec.kind != LEARNER_TRPO && pl.lds.bytes > 48 * 1024 && !(h->ppo_attr_mask & bit)) {   // (function attributes are per device: once per handle)
        e = hipFuncSetAttribute(ppo_grad_kernel(relu, head).fn, hipFuncAttributeMaxDynamicSharedMemorySize, EV2G_PPO_LDS_LIMIT);
        if (e == hipSuccess) h->ppo_attr_mask |= bit;
    }
    if (e != hipSuccess) return fail(h, EV2G_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return EV2G_OK;
}

// a create entry (ev2g_ppo_create, ev2g_a2c_create; CONFIG: its kind's): checks, then plans, allocates and binds a learner with the config's spec
// (a template needs C++ linkage inside this file's extern "C" block)
extern "C++" template <class CONFIG>
static int learner_create(ev2g_handle *h, ev2g_acpolicy *ac, const char *who, const CONFIG *cfg, ev2g_ppo **out) {
    if (!h || !out) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    *out = nullptr;
    if (!cfg) return fail(h, EV2G_ERR_ARG, std::string(who) + ": cfg is null");
    if (int rc = ac_check(h, ac, who)) return rc;
    if (int rc = fields_check(h, who, learner_fields(*cfg))) return rc;
    if (ac->learner) return fail(h, EV2G_ERR_STATE, std::string(who) + ": the policy already has a learner");
    const AcPlan &a = ac->plan;
    const PpoPlan plan = plan_ppo(a.d_in, a.h1, a.h2, a.v1, a.v2, a.d_out);
    if (plan.err) return fail(h, plan.err, plan.refusal);
    ev2g_ppo *p = new ev2g_ppo();
    p->spec = learner_spec(*cfg); p->plan = plan;
    p->n_blocks = (plan.n_params + 255) / 256;
    const int rc = owned_created(h, &ev2g_handle::ppos, p, ppo_device_stage(h, p, ac, who), out);
    if (!rc) { p->ac = ac; ac->learner = p; }
    return rc;
}

// the gradient of either kind: the advantage statistics if asked for, the gradient kernel with the learner's head, the reduction
// (old_lp: null from the entries of a head that does not read it)
static int learner_grad(ev2g_handle *h, ev2g_ppo *p, const char *who, int kind, const float *obs, const float *actions, const float *old_lp,
                        const float *adv, const float *ret, const int32_t *idx, int B, float *stats) {
    if (int rc = learner_check(h, p, who, kind)) return rc;
    const LearnerSpec &s = p->spec;
    if (!obs || !actions || (s.reads_old_lp && !old_lp) || !adv || !ret || !idx) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (B < 1) return fail(h, EV2G_ERR_ARG, std::string(who) + ": B must be at least 1");
    if (s.one_row_norm_refused && s.hyper.normalize && B == 1)
        return fail(h, EV2G_ERR_ARG, std::string(who) + ": normalize_advantage needs B >= 2 (the unbiased std of one advantage is undefined)");
    const PpoPlan &pl = p->plan;
    const PpoHyper &hp = s.hyper;
    if (hp.normalize && B > 1) hipLaunchKernelGGL(ev2g_ppo_advstat_kernel, dim3(1), dim3(1024), 0, h->stream, adv, (const int *)idx, B, p->advstat);
    const int chunks = (B + EV2G_PPO_ROWS - 1) / EV2G_PPO_ROWS, n_wg = chunks < pl.grid_cap ? chunks : pl.grid_cap;
    const LaunchDims dims{dim3((unsigned)n_wg), pl.lds.bytes, h->stream};
    ppo_grad_kernel(p->ac->relu, s.head).launch(dims, p->ac->dev, p->dev, pl.lds, hp, obs, actions, old_lp, adv, ret, (const int *)idx, B, (const double *)p->advstat,
                                                p->work, p->stat_part);
    hipLaunchKernelGGL(ev2g_ppo_reduce_kernel, dim3((unsigned)p->n_blocks), dim3(256), 0, h->stream, p->map, (const float *)p->work,
                       (const double *)p->stat_part, n_wg, B, hp, p->dev.log_std, p->grad, p->norm_part, stats);
    HIPCHK(h, hipGetLastError());
    p->have_grad = true;
    return EV2G_OK;
}

// clip_grad_norm_, the spec's optimiser, repack
static int learner_apply(ev2g_handle *h, ev2g_ppo *p, const char *who, int kind) {
    if (int rc = learner_check(h, p, who, kind)) return rc;
    const LearnerSpec &s = p->spec;
    if (!p->have_grad) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no gradient to apply (" + s.grad_entry + " first)");
    p->t += 1;
    if (s.optimiser == LEARNER_RMSPROP)
        hipLaunchKernelGGL(ev2g_a2c_apply_kernel, dim3((unsigned)p->n_blocks), dim3(256), 0, h->stream, p->map, (const float *)p->grad,
                           (const double *)p->norm_part, p->n_blocks, (float)s.max_grad_norm, rms_step(s.lr, s.alpha, s.eps), p->theta, p->v);
    else
        hipLaunchKernelGGL(ev2g_ppo_apply_kernel, dim3((unsigned)p->n_blocks), dim3(256), 0, h->stream, p->map, (const float *)p->grad,
                           (const double *)p->norm_part, p->n_blocks, (float)s.max_grad_norm, adam_step(s.lr, s.beta1, s.beta2, s.eps, p->t), p->theta, p->m,
                           p->v);
    HIPCHK(h, hipGetLastError());
    p->have_grad = false;
    return EV2G_OK;
}

int ev2g_ppo_create(ev2g_handle *h, ev2g_acpolicy *ac, const ev2g_ppo_config *cfg, ev2g_ppo **out) { return learner_create(h, ac, "ev2g_ppo_create", cfg, out); }

int ev2g_a2c_create(ev2g_handle *h, ev2g_acpolicy *ac, const ev2g_a2c_config *cfg, ev2g_ppo **out) { return learner_create(h, ac, "ev2g_a2c_create", cfg, out); }

void ev2g_ppo_destroy(ev2g_handle *h, ev2g_ppo *ppo) { owned_destroy(h, &ev2g_handle::ppos, ppo, ppo_free); }

int ev2g_ppo_set_rates(ev2g_handle *h, ev2g_ppo *p, double lr, double clip_range) {
    if (int rc = learner_check(h, p, "ev2g_ppo_set_rates", LEARNER_PPO)) return rc;
    if (int rc = fields_check(h, "ev2g_ppo_set_rates", ppo_rate_fields(lr, clip_range))) return rc;
    p->spec.lr = lr; p->spec.hyper.clip = (float)clip_range;
    return EV2G_OK;
}

int ev2g_a2c_set_rate(ev2g_handle *h, ev2g_ppo *p, double lr) {
    if (int rc = learner_check(h, p, "ev2g_a2c_set_rate", LEARNER_A2C)) return rc;
    if (int rc = fields_check(h, "ev2g_a2c_set_rate", a2c_rate_fields(lr))) return rc;
    p->spec.lr = lr;
    return EV2G_OK;
}

int ev2g_ppo_grad(ev2g_handle *h, ev2g_ppo *ppo, const float *obs, const float *actions, const float *old_log_prob, const float *advantages,
                  const float *returns, const int32_t *idx, int B, float *stats) {
    return learner_grad(h, ppo, "ev2g_ppo_grad", LEARNER_PPO, obs, actions, old_log_prob, advantages, returns, idx, B, stats);
}

int ev2g_ppo_apply(ev2g_handle *h, ev2g_ppo *ppo) { return learner_apply(h, ppo, "ev2g_ppo_apply", LEARNER_PPO); }

int ev2g_ppo_minibatch(ev2g_handle *h, ev2g_ppo *ppo, const float *obs, const float *actions, const float *old_log_prob, const float *advantages,
                       const float *returns, const int32_t *idx, int B, float *stats) {
    if (int rc = learner_grad(h, ppo, "ev2g_ppo_minibatch", LEARNER_PPO, obs, actions, old_log_prob, advantages, returns, idx, B, stats)) return rc;
    return learner_apply(h, ppo, "ev2g_ppo_minibatch", LEARNER_PPO);
}

int ev2g_a2c_grad(ev2g_handle *h, ev2g_ppo *learner, const float *obs, const float *actions, const float *advantages, const float *returns,
                  const int32_t *idx, int B, float *stats) {
    return learner_grad(h, learner, "ev2g_a2c_grad", LEARNER_A2C, obs, actions, nullptr, advantages, returns, idx, B, stats);
}

int ev2g_a2c_apply(ev2g_handle *h, ev2g_ppo *learner) { return learner_apply(h, learner, "ev2g_a2c_apply", LEARNER_A2C); }

int ev2g_a2c_update(ev2g_handle *h, ev2g_ppo *learner, const float *obs, const float *actions, const float *advantages, const float *returns,
                    const int32_t *idx, int B, float *stats) {
    if (int rc = learner_grad(h, learner, "ev2g_a2c_update", LEARNER_A2C, obs, actions, nullptr, advantages, returns, idx, B, stats)) return rc;
    return learner_apply(h, learner, "ev2g_a2c_update", LEARNER_A2C);
}

// a flat [n_params] device buffer into the thirteen host arrays
static int ppo_read_flat(ev2g_handle *h, const PpoPlan &pl, const float *src, float *const out[EV2G_PPO_ARRAYS]) {
    for (int i = 0; i < EV2G_PPO_ARRAYS; i++)
        if (out[i])
            HIPCHK(h, hipMemcpyAsync(out[i], src + pl.off[i], (size_t)(pl.off[i + 1] - pl.off[i]) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

int ev2g_ppo_get_grads(ev2g_handle *h, ev2g_ppo *ppo, float *pi_W1, float *pi_b1, float *pi_W2, float *pi_b2, float *vf_W1, float *vf_b1,
                       float *vf_W2, float *vf_b2, float *action_W, float *action_b, float *value_W, float *value_b, float *log_std) {
    if (int rc = ppo_check(h, ppo, "ev2g_ppo_get_grads")) return rc;
    float *const out[EV2G_PPO_ARRAYS] = {pi_W1, pi_b1, pi_W2, pi_b2, vf_W1, vf_b1, vf_W2, vf_b2, action_W, action_b, value_W, value_b, log_std};
    for (float *o : out)
        if (!o) return fail(h, EV2G_ERR_ARG, "ev2g_ppo_get_grads: null argument");
    return ppo_read_flat(h, ppo->plan, ppo->grad, out);
}

int ev2g_ppo_sync(ev2g_handle *h, ev2g_ppo *ppo) {
    if (int rc = ppo_check(h, ppo, "ev2g_ppo_sync")) return rc;
    std::vector<float> ls((size_t)ppo->ac->dev.d_out);
    HIPCHK(h, hipMemcpyAsync(ls.data(), ppo->dev.log_std, ls.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ac_upload_log_std(h, ppo->ac, ls.data(), "ev2g_ppo_sync");
}

int ev2g_ac_get_weights(ev2g_handle *h, ev2g_acpolicy *ac, float *pi_W1, float *pi_b1, float *pi_W2, float *pi_b2, float *vf_W1, float *vf_b1,
                        float *vf_W2, float *vf_b2, float *action_W, float *action_b, float *value_W, float *value_b, float *log_std) {
    if (int rc = ac_check(h, ac, "ev2g_ac_get_weights")) return rc;
    float *const out[EV2G_PPO_ARRAYS] = {pi_W1, pi_b1, pi_W2, pi_b2, vf_W1, vf_b1, vf_W2, vf_b2, action_W, action_b, value_W, value_b, log_std};
    for (float *o : out)
        if (!o) return fail(h, EV2G_ERR_ARG, "ev2g_ac_get_weights: null argument");
    if (ac->learner) return ppo_read_flat(h, ac->learner->plan, ac->learner->theta, out);
    if (int rc = ac_read_images(h, ac, out)) return rc;
    std::copy(ac->log_std.begin(), ac->log_std.end(), log_std);
    return EV2G_OK;
}

int ev2g_host_adam(float *theta, float *m, float *v, const float *g, int64_t n, int64_t t, double lr, double beta1, double beta2, double eps) {
    if (!theta || !m || !v || !g || n < 0 || t < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_adam: null argument, n < 0 or t < 1");
    if (!std::isfinite(lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0))
        return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_adam: lr must be finite, the betas in [0, 1), eps > 0");
    const AdamStep a = adam_step(lr, beta1, beta2, eps, (long long)t);
    for (int64_t i = 0; i < n; i++) ev2g_adam_elem(theta + i, m + i, v + i, g[i], a);
    return EV2G_OK;
}

int ev2g_host_ppo_head(const float *mean, const float *value, const float *actions, const float *log_std, const float *old_log_prob,
                       const float *advantages, const float *returns, int B, int P, const ev2g_ppo_config *cfg, float *d_mean, float *d_value,
                       float *d_log_std, float *stats) {
    if (!mean || !value || !actions || !log_std || !old_log_prob || !advantages || !returns || !cfg || !d_mean || !d_value || !d_log_std || !stats)
        return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_ppo_head: null argument");
    if (B < 1 || P < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_ppo_head: B and P must be positive");
    learner_host_head(learner_spec(*cfg), mean, value, actions, log_std, old_log_prob, advantages, returns, B, P, d_mean, d_value, d_log_std, stats);
    return EV2G_OK;
}

int ev2g_host_rmsprop(float *theta, float *sq, const float *g, int64_t n, double lr, double alpha, double eps) {
    if (!theta || !sq || !g || n < 0) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_rmsprop: null argument or n < 0");
    if (!std::isfinite(lr) || !(alpha >= 0.0 && alpha < 1.0) || !(eps > 0.0))
        return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_rmsprop: lr must be finite, alpha in [0, 1), eps > 0");
    const RmsStep s = rms_step(lr, alpha, eps);
    for (int64_t i = 0; i < n; i++) ev2g_rmsprop_elem(theta + i, sq + i, g[i], s);
    return EV2G_OK;
}

int ev2g_host_a2c_head(const float *mean, const float *value, const float *actions, const float *log_std, const float *advantages,
                       const float *returns, int B, int P, const ev2g_a2c_config *cfg, float *d_mean, float *d_value, float *d_log_std, float *stats) {
    if (!mean || !value || !actions || !log_std || !advantages || !returns || !cfg || !d_mean || !d_value || !d_log_std || !stats)
        return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_a2c_head: null argument");
    if (B < 1 || P < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_a2c_head: B and P must be positive");
    const LearnerSpec spec = learner_spec(*cfg);
    if (spec.one_row_norm_refused && spec.hyper.normalize && B == 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_a2c_head: normalize_advantage needs B >= 2");
    learner_host_head(spec, mean, value, actions, log_std, nullptr, advantages, returns, B, P, d_mean, d_value, d_log_std, stats);
    return EV2G_OK;
}

// ---- the TRPO learner (ev2g_trpo.h): a third kind of ev2g_ppo ----
int ev2g_trpo_query(int d_in, int h1, int h2, int v1, int v2, int d_out, ev2g_trpo_info *info) {
    if (!info) return fail(nullptr, EV2G_ERR_ARG, "ev2g_trpo_query: info is null");
    const TrpoPlan p = plan_trpo(d_in, h1, h2, v1, v2, d_out);
    if (p.err) return fail(nullptr, p.err, p.refusal);
    info->lds_bytes = (int64_t)p.lds.bytes; info->workspace_bytes = (int64_t)(p.ppo.workspace_bytes + p.vector_bytes);
    info->grid_cap = p.ppo.grid_cap; info->n_params = p.ppo.n_params; info->n_actor = p.n_actor;
    return EV2G_OK;
}

// the kernels of one activation (ev2g_trpo_create sets their dynamic-LDS attribute)
struct TrpoKernels { const void *fn[4]; };
extern "C++" template <int ACT>
static TrpoKernels trpo_kernels_of() {
    return {{(const void *)ev2g_trpo_policy_kernel<ACT, EV2G_TRPO_GRAD>, (const void *)ev2g_trpo_policy_kernel<ACT, EV2G_TRPO_FVP>,
             (const void *)ev2g_trpo_policy_kernel<ACT, EV2G_TRPO_EVAL>, (const void *)ev2g_trpo_value_kernel<ACT>}};
}
// mode: EV2G_TRPO_GRAD / _FVP / _EVAL, or 3: the critic's kernel
static void trpo_launch_rows(ev2g_handle *h, ev2g_ppo *p, int mode, int n_wg, const TrpoArgs &a) {
    const dim3 grid((unsigned)n_wg), block(EV2G_PPO_BLOCK);
    const size_t lds = p->tplan.lds.bytes;
    const AcDev &ac = p->ac->dev;
    const TrpoLds &L = p->tplan.lds;
#define EV2G_TRPO_LAUNCH(ACT) \
    switch (mode) { \
    case EV2G_TRPO_GRAD: hipLaunchKernelGGL((ev2g_trpo_policy_kernel<ACT, EV2G_TRPO_GRAD>), grid, block, lds, h->stream, ac, p->dev, L, a); break; \
    case EV2G_TRPO_FVP: hipLaunchKernelGGL((ev2g_trpo_policy_kernel<ACT, EV2G_TRPO_FVP>), grid, block, lds, h->stream, ac, p->dev, L, a); break; \
    case EV2G_TRPO_EVAL: hipLaunchKernelGGL((ev2g_trpo_policy_kernel<ACT, EV2G_TRPO_EVAL>), grid, block, lds, h->stream, ac, p->dev, L, a); break; \
    default: hipLaunchKernelGGL((ev2g_trpo_value_kernel<ACT>), grid, block, lds, h->stream, ac, p->dev, L, a); break; \
    }
    if (p->ac->relu) { EV2G_TRPO_LAUNCH(EV2G_AC_RELU) } else { EV2G_TRPO_LAUNCH(EV2G_AC_TANH) }
#undef EV2G_TRPO_LAUNCH
}

static int trpo_device_stage(ev2g_handle *h, ev2g_ppo *p, const char *who) {
    const TrpoPlan &tp = p->tplan;
    const size_t n = (size_t)tp.n_actor;
    double **f64[] = {&p->tg, &p->tx, &p->tr, &p->tp, &p->thv};
    for (double **d : f64)
        if (int rc = dalloc(h, p->allocs, n, d)) return rc;
    if (int rc = dalloc(h, p->allocs, (size_t)tp.ppo.grid_cap * 2, &p->tpart)) return rc;
    if (int rc = dalloc(h, p->allocs, n, &p->theta0)) return rc;
    if (int rc = dalloc(h, p->allocs, 1, &p->tstate)) return rc;
    const auto tab = ac_params(tp.ppo.ac);
    for (int k = 0; k < EV2G_TRPO_ACTOR_ARRAYS; k++)
        if (tab[(size_t)tp.arr[k]].slot != AC_NO_IMAGE)
            if (int rc = dalloc(h, p->allocs, tab[(size_t)tp.arr[k]].img_floats, &p->dimg[k])) return rc;
    p->tmap = trpo_map(tp, p->dimg);
    p->n_ablocks = (tp.n_actor + 255) / 256;
    const int relu = p->ac->relu ? 1 : 0;
    if (tp.lds.bytes > 48 * 1024 && !(h->trpo_attr_mask & (1u << relu))) {
        const TrpoKernels k = relu ? trpo_kernels_of<EV2G_AC_RELU>() : trpo_kernels_of<EV2G_AC_TANH>();
        for (const void *fn : k.fn) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, EV2G_PPO_LDS_LIMIT);
            if (e != hipSuccess) return fail(h, EV2G_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
        }
        h->trpo_attr_mask |= 1u << relu;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

int ev2g_trpo_create(ev2g_handle *h, ev2g_acpolicy *ac, const ev2g_trpo_config *cfg, ev2g_ppo **out) {
    if (int rc = learner_create(h, ac, "ev2g_trpo_create", cfg, out)) return rc;
    ev2g_ppo *p = *out;
    p->trpo = trpo_spec(*cfg);
    p->tplan = plan_trpo(ac->plan.d_in, ac->plan.h1, ac->plan.h2, ac->plan.v1, ac->plan.v2, ac->plan.d_out);
    if (int rc = trpo_device_stage(h, p, "ev2g_trpo_create")) {
        owned_destroy(h, &ev2g_handle::ppos, p, ppo_free);
        *out = nullptr;
        return rc;
    }
    return EV2G_OK;
}

int ev2g_trpo_set_rate(ev2g_handle *h, ev2g_ppo *p, double lr) {
    if (int rc = learner_check(h, p, "ev2g_trpo_set_rate", LEARNER_TRPO)) return rc;
    if (int rc = fields_check(h, "ev2g_trpo_set_rate", trpo_rate_fields(lr))) return rc;
    p->spec.lr = lr; p->trpo.lr = lr;
    return EV2G_OK;
}

static int trpo_wgs(const ev2g_ppo *p, int B) {
    const int chunks = (B + EV2G_PPO_ROWS - 1) / EV2G_PPO_ROWS;
    return chunks < p->tplan.ppo.grid_cap ? chunks : p->tplan.ppo.grid_cap;
}

// mu0 [B, P]: regrown when B * P grows
static int trpo_rows_block(ev2g_handle *h, ev2g_ppo *p, int B) {
    const size_t need = (size_t)B * (size_t)p->ac->dev.d_out;
    if (p->mu0_elems >= need) return EV2G_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    free_pool(p->swap_allocs); p->mu0 = nullptr; p->mu0_elems = 0;
    if (int rc = dalloc(h, p->swap_allocs, need, &p->mu0)) return rc;
    p->mu0_elems = need;
    return EV2G_OK;
}

// the queue of g, J(theta0), mu0: the advantage statistics if asked for, the GRAD launch, the reduction
static int trpo_queue_grad(ev2g_handle *h, ev2g_ppo *p, TrpoArgs &a) {
    const int B = a.B, n_wg = trpo_wgs(p, B);
    if (int rc = trpo_rows_block(h, p, B)) return rc;
    if (a.normalize && B > 1) hipLaunchKernelGGL(ev2g_ppo_advstat_kernel, dim3(1), dim3(1024), 0, h->stream, a.adv, a.idx, B, p->advstat);
    a.advstat = p->advstat; a.work = p->work; a.part = p->tpart; a.mu0 = p->mu0; a.st = p->tstate; a.gate = EV2G_TRPO_GATE_NONE;
    trpo_launch_rows(h, p, EV2G_TRPO_GRAD, n_wg, a);
    hipLaunchKernelGGL(ev2g_trpo_reduce_kernel<float>, dim3((unsigned)p->n_ablocks), dim3(256), 0, h->stream, p->map, p->tmap, (const float *)p->work, n_wg, 0,
                       (const float *)nullptr, 0.0, p->tg, (float *)nullptr, p->grad, (const double *)p->tpart, B, p->tstate, EV2G_TRPO_GATE_NONE);
    return EV2G_OK;
}

// H v for the float64 vector v -> p->thv (gate: the launches return at once when the solve has ended)
static void trpo_queue_fvp(ev2g_handle *h, ev2g_ppo *p, TrpoArgs a, const double *v, int gate) {
    const int n_wg = trpo_wgs(p, a.B);
    hipLaunchKernelGGL(ev2g_trpo_dir_kernel<double>, dim3((unsigned)p->n_ablocks), dim3(256), 0, h->stream, p->tmap, v, (const TrpoState *)p->tstate, gate);
    a.gate = gate;
    trpo_launch_rows(h, p, EV2G_TRPO_FVP, n_wg, a);
    hipLaunchKernelGGL(ev2g_trpo_reduce_kernel<double>, dim3((unsigned)p->n_ablocks), dim3(256), 0, h->stream, p->map, p->tmap, (const float *)p->work, n_wg, 1, v,
                       p->trpo.cg_damping, p->thv, (float *)nullptr, (float *)nullptr, (const double *)p->tpart, a.B, p->tstate, gate);
}

static TrpoArgs trpo_args(const ev2g_ppo *p, const float *obs, const float *actions, const float *old_lp, const float *adv, const float *ret, const int32_t *idx,
                          int B) {
    TrpoArgs a{};
    a.obs = obs; a.actions = actions; a.old_lp = old_lp; a.adv = adv; a.ret = ret; a.idx = (const int *)idx; a.B = B; a.normalize = p->trpo.normalize;
    a.advstat = p->advstat; a.work = p->work; a.part = p->tpart; a.mu0 = p->mu0; a.ls0 = p->theta0;   // (log_std leads a flat actor vector)
    a.dw1 = p->dimg[1]; a.db1 = p->dimg[2]; a.dw2 = p->dimg[3]; a.db2 = p->dimg[4]; a.dw3 = p->dimg[5]; a.db3 = p->dimg[6];
    a.st = p->tstate; a.gate = EV2G_TRPO_GATE_NONE;
    return a;
}

int ev2g_trpo_grad(ev2g_handle *h, ev2g_ppo *p, const float *obs, const float *actions, const float *old_lp, const float *adv, const int32_t *idx, int B,
                   double *objective) {
    if (int rc = learner_check(h, p, "ev2g_trpo_grad", LEARNER_TRPO)) return rc;
    if (!obs || !actions || !old_lp || !adv || !idx) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_grad: null argument");
    if (B < 1) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_grad: B must be at least 1");
    TrpoArgs a = trpo_args(p, obs, actions, old_lp, adv, nullptr, idx, B);
    if (int rc = trpo_queue_grad(h, p, a)) return rc;
    if (objective) HIPCHK(h, hipMemcpyAsync(objective, &p->tstate->J0, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_trpo_fvp(ev2g_handle *h, ev2g_ppo *p, const float *obs, const int32_t *idx, int B, const float *v, float *Hv) {
    if (int rc = learner_check(h, p, "ev2g_trpo_fvp", LEARNER_TRPO)) return rc;
    if (!obs || !idx || !v || !Hv) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_fvp: null argument");
    if (B < 1) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_fvp: B must be at least 1");
    const TrpoArgs a = trpo_args(p, obs, nullptr, nullptr, nullptr, nullptr, idx, B);
    const int n_wg = trpo_wgs(p, B);
    hipLaunchKernelGGL(ev2g_trpo_dir_kernel<float>, dim3((unsigned)p->n_ablocks), dim3(256), 0, h->stream, p->tmap, v, (const TrpoState *)p->tstate,
                       EV2G_TRPO_GATE_NONE);
    trpo_launch_rows(h, p, EV2G_TRPO_FVP, n_wg, a);
    hipLaunchKernelGGL(ev2g_trpo_reduce_kernel<float>, dim3((unsigned)p->n_ablocks), dim3(256), 0, h->stream, p->map, p->tmap, (const float *)p->work, n_wg, 1, v,
                       p->trpo.cg_damping, (double *)nullptr, Hv, (float *)nullptr, (const double *)p->tpart, B, p->tstate, EV2G_TRPO_GATE_NONE);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_trpo_policy_step(ev2g_handle *h, ev2g_ppo *p, const float *obs, const float *actions, const float *old_lp, const float *adv, const int32_t *idx,
                          int B) {
    if (int rc = learner_check(h, p, "ev2g_trpo_policy_step", LEARNER_TRPO)) return rc;
    if (!obs || !actions || !old_lp || !adv || !idx) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_policy_step: null argument");
    if (B < 1) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_policy_step: B must be at least 1");
    const TrpoSpec &s = p->trpo;
    TrpoArgs a = trpo_args(p, obs, actions, old_lp, adv, nullptr, idx, B);
    if (int rc = trpo_queue_grad(h, p, a)) return rc;
    const int n = p->tplan.n_actor, n_wg = trpo_wgs(p, B);
    const dim3 one(1), cg(EV2G_TRPO_CG_BLOCK), ab((unsigned)p->n_ablocks);
    hipLaunchKernelGGL(ev2g_trpo_cg_init_kernel, one, cg, 0, h->stream, n, (const double *)p->tg, p->tx, p->tr, p->tp, p->tstate);
    for (int i = 0; i < s.cg_max_steps; i++) {
        trpo_queue_fvp(h, p, a, p->tp, EV2G_TRPO_GATE_CG);
        hipLaunchKernelGGL(ev2g_trpo_cg_step_kernel, one, cg, 0, h->stream, n, (const double *)p->thv, p->tx, p->tr, p->tp, p->tstate, i == s.cg_max_steps - 1 ? 1 : 0);
    }
    trpo_queue_fvp(h, p, a, p->tx, EV2G_TRPO_GATE_NONE);
    hipLaunchKernelGGL(ev2g_trpo_stepsize_kernel, one, cg, 0, h->stream, p->map, p->tmap, (const double *)p->tx, (const double *)p->thv, s.target_kl,
                       (const float *)p->theta, p->theta0, p->tstate);
    a.gate = EV2G_TRPO_GATE_LS;
    for (int k = 0; k < s.ls_max_iter; k++) {
        hipLaunchKernelGGL(ev2g_trpo_candidate_kernel, ab, dim3(256), 0, h->stream, p->map, p->tmap, (const double *)p->tx, (const float *)p->theta0, p->theta,
                           (const TrpoState *)p->tstate);
        trpo_launch_rows(h, p, EV2G_TRPO_EVAL, n_wg, a);
        hipLaunchKernelGGL(ev2g_trpo_decide_kernel, one, cg, 0, h->stream, p->map, p->tmap, (const double *)p->tpart, n_wg, B, s.target_kl, s.shrink,
                           k == s.ls_max_iter - 1 ? 1 : 0, (const float *)p->theta0, p->theta, p->tstate);
    }
    HIPCHK(h, hipGetLastError());
    p->have_step = true;
    return EV2G_OK;
}

int ev2g_trpo_critic_minibatch(ev2g_handle *h, ev2g_ppo *p, const float *obs, const float *returns, const int32_t *idx, int B, float *value_loss) {
    if (int rc = learner_check(h, p, "ev2g_trpo_critic_minibatch", LEARNER_TRPO)) return rc;
    if (!obs || !returns || !idx) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_critic_minibatch: null argument");
    if (B < 1) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_critic_minibatch: B must be at least 1");
    const TrpoArgs a = trpo_args(p, obs, nullptr, nullptr, nullptr, returns, idx, B);
    const int n_wg = trpo_wgs(p, B);
    trpo_launch_rows(h, p, 3, n_wg, a);
    hipLaunchKernelGGL(ev2g_trpo_vreduce_kernel, dim3((unsigned)p->n_blocks), dim3(256), 0, h->stream, p->map, (const float *)p->work, (const double *)p->tpart, n_wg,
                       B, p->grad, value_loss);
    p->t += 1;
    hipLaunchKernelGGL(ev2g_trpo_vapply_kernel, dim3((unsigned)p->n_blocks), dim3(256), 0, h->stream, p->map, (const float *)p->grad,
                       adam_step(p->spec.lr, p->spec.beta1, p->spec.beta2, p->spec.eps, p->t), p->theta, p->m, p->v);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_trpo_get_report(ev2g_handle *h, ev2g_ppo *p, ev2g_trpo_report *report) {
    if (int rc = learner_check(h, p, "ev2g_trpo_get_report", LEARNER_TRPO)) return rc;
    if (!report) return fail(h, EV2G_ERR_ARG, "ev2g_trpo_get_report: report is null");
    if (!p->have_step) return fail(h, EV2G_ERR_STATE, "ev2g_trpo_get_report: no policy step yet (ev2g_trpo_policy_step first)");
    TrpoState st;
    HIPCHK(h, hipMemcpyAsync(&st, p->tstate, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    report->cg_iterations = st.cg_iters; report->line_search_tries = st.ls_tries; report->accepted = st.accepted; report->failed = st.failed;
    report->objective_before = st.J0; report->objective_after = st.J1; report->kl = st.kl; report->beta = st.beta; report->c = st.c; report->xHx = st.xHx;
    return EV2G_OK;
}

int ev2g_trpo_get_direction(ev2g_handle *h, ev2g_ppo *p, double *x, double *g) {
    if (int rc = learner_check(h, p, "ev2g_trpo_get_direction", LEARNER_TRPO)) return rc;
    if (!p->have_step) return fail(h, EV2G_ERR_STATE, "ev2g_trpo_get_direction: no policy step yet (ev2g_trpo_policy_step first)");
    const size_t bytes = (size_t)p->tplan.n_actor * sizeof(double);
    if (x) HIPCHK(h, hipMemcpyAsync(x, p->tx, bytes, hipMemcpyDeviceToHost, h->stream));
    if (g) HIPCHK(h, hipMemcpyAsync(g, p->tg, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

int ev2g_host_trpo_cg_step(double *x, double *r, double *p, const double *Hp, int64_t n, double *rho, int last, int32_t *done) {
    if (!x || !r || !p || !Hp || !rho || !done || n < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_trpo_cg_step: null argument or n < 1");
    *done = trpo_host_cg_step(x, r, p, Hp, (int)n, rho, last);
    return EV2G_OK;
}

int ev2g_host_trpo_rows(const float *mean, const float *mean0, const float *actions, const float *log_std, const float *log_std0, const float *old_log_prob,
                        const float *advantages, int B, int P, int normalize_advantage, double *j, double *kl) {
    if (!mean || !mean0 || !actions || !log_std || !log_std0 || !old_log_prob || !advantages || !j || !kl)
        return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_trpo_rows: null argument");
    if (B < 1 || P < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_trpo_rows: B and P must be positive");
    trpo_host_rows(mean, mean0, actions, log_std, log_std0, old_log_prob, advantages, B, P, normalize_advantage, j, kl);
    return EV2G_OK;
}

// ---- the TD3 / DDPG learner (ev2g_td3.h) and the replay ring's sampler ----
static int td3_check(ev2g_handle *h, ev2g_td3 *t, const char *who) {
    if (int rc = owned_check(h, &ev2g_handle::td3s, t, "learner", who, false)) return rc;
    if (!t->policy) return fail(h, EV2G_ERR_STATE, std::string(who) + ": the learner's policy was destroyed without its handle");   // (its images are gone)
    return EV2G_OK;
}

static void td3_gemm(ev2g_handle *h, const Td3Gemm &g, int nz) {
    const dim3 grid((unsigned)((g.N + EV2G_TD3_TILE - 1) / EV2G_TD3_TILE), (unsigned)((g.M + EV2G_TD3_TILE - 1) / EV2G_TD3_TILE), (unsigned)nz);
    hipLaunchKernelGGL(ev2g_td3_gemm_kernel, grid, dim3(EV2G_TD3_TILE, EV2G_TD3_TILE), 0, h->stream, g);
}
static unsigned td3_blocks(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 1024); }

// nz networks of one kind (parameter blocks th + z zP, the six arrays at off[]), all reading x [B, k0]: the two hidden layers into H1 / H2
// (z strides B h1 / B h2) and the output layer [B, n_out] into O (z stride B n_out) under out_epi
struct Td3Net { const float *th; long long zP; const int *off; int k0, h1, h2, n_out; float *H1, *H2, *O; };
static void td3_forward(ev2g_handle *h, const Td3Net &n, const float *x, int B, int out_epi, int nz) {
    const long long z1 = (long long)B * n.h1, z2 = (long long)B * n.h2, zo = (long long)B * n.n_out;
    Td3Gemm g{};
    g.M = B; g.sak = 1; g.sbk = 1; g.zB = n.zP; g.zbias = n.zP;
    g.A = x; g.zA = 0; g.sam = n.k0; g.K = n.k0; g.N = n.h1; g.Bm = n.th + n.off[0]; g.sbn = n.k0; g.bias = n.th + n.off[1]; g.C = n.H1; g.ldc = n.h1; g.zC = z1;
    g.epi = TD3_EPI_BIAS_RELU;
    td3_gemm(h, g, nz);
    g.A = n.H1; g.zA = z1; g.sam = n.h1; g.K = n.h1; g.N = n.h2; g.Bm = n.th + n.off[2]; g.sbn = n.h1; g.bias = n.th + n.off[3]; g.C = n.H2; g.ldc = n.h2; g.zC = z2;
    td3_gemm(h, g, nz);
    g.A = n.H2; g.zA = z2; g.sam = n.h2; g.K = n.h2; g.N = n.n_out; g.Bm = n.th + n.off[4]; g.sbn = n.h2; g.bias = n.th + n.off[5]; g.C = n.O; g.ldc = n.n_out; g.zC = zo;
    g.epi = out_epi;
    td3_gemm(h, g, nz);
}
// the weight gradient of nz layers: grad_w[z] [rows, cols] = delta[z]^T in[z] (k: the batch rows ascending) and grad_b[z] [rows] = the column sums of delta[z]
static void td3_wgrad(ev2g_handle *h, int B, const float *delta, long long zd, int rows, const float *in, long long zin, int cols, float *grad_w, float *grad_b,
                      long long zP, int nz) {
    Td3Gemm g{};
    g.M = rows; g.N = cols; g.K = B; g.A = delta; g.zA = zd; g.sam = 1; g.sak = rows; g.Bm = in; g.zB = zin; g.sbk = cols; g.sbn = 1;
    g.C = grad_w; g.ldc = cols; g.zC = zP; g.epi = TD3_EPI_NONE; g.acc64 = 1;
    td3_gemm(h, g, nz);
    hipLaunchKernelGGL(ev2g_td3_colsum_kernel, dim3((unsigned)((rows + 15) / 16), (unsigned)nz), dim3(256), 0, h->stream, delta, zd, B, rows, grad_b, zP);
}
// backward data of nz layers: out[z] [B, cols] = delta[z] [B, k] W[z][:, 0 .. cols) (row stride ldw), masked by H[z] > 0 when H is given
static void td3_bdata(ev2g_handle *h, int B, const float *delta, long long zd, int k, const float *W, long long zW, int ldw, int cols, const float *H, long long zH,
                      float *out, long long zout, int nz) {
    Td3Gemm g{};
    g.M = B; g.N = cols; g.K = k; g.A = delta; g.zA = zd; g.sam = k; g.sak = 1; g.Bm = W; g.zB = zW; g.sbk = ldw; g.sbn = 1;
    g.C = out; g.ldc = cols; g.zC = zout; g.H = H; g.ldh = cols; g.zH = zH; g.epi = H ? TD3_EPI_MASK : TD3_EPI_NONE;
    td3_gemm(h, g, nz);
}
// backprop from dO [nz][B, n_out] (the delta at the output layer's pre-activation) through the networks td3_forward ran: the hidden deltas into
// D2 / D1, the six gradients into grad + z zP (grad null: none), and -- dX not null -- the delta of input columns [x_col0, x_col0 + x_cols) into
// dX [nz][B, x_cols]
static void td3_backward(ev2g_handle *h, const Td3Net &n, const float *x, int B, const float *dO, float *D2, float *D1, float *grad, float *dX, int x_col0,
                         int x_cols, int nz) {
    const long long z1 = (long long)B * n.h1, z2 = (long long)B * n.h2, zo = (long long)B * n.n_out;
    if (grad) td3_wgrad(h, B, dO, zo, n.n_out, n.H2, z2, n.h2, grad + n.off[4], grad + n.off[5], n.zP, nz);
    td3_bdata(h, B, dO, zo, n.n_out, n.th + n.off[4], n.zP, n.h2, n.h2, n.H2, z2, D2, z2, nz);
    if (grad) td3_wgrad(h, B, D2, z2, n.h2, n.H1, z1, n.h1, grad + n.off[2], grad + n.off[3], n.zP, nz);
    td3_bdata(h, B, D2, z2, n.h2, n.th + n.off[2], n.zP, n.h1, n.h1, n.H1, z1, D1, z1, nz);
    if (grad) td3_wgrad(h, B, D1, z1, n.h1, x, 0, n.k0, grad + n.off[0], grad + n.off[1], n.zP, nz);
    if (dX) td3_bdata(h, B, D1, z1, n.h1, n.th + n.off[0] + x_col0, n.zP, n.k0, x_cols, nullptr, 0, dX, (long long)B * x_cols, nz);
}
static Td3Net td3_actor_net(const ev2g_td3 *t, const float *params) {
    const Td3Plan &p = t->plan;
    return {params, 0, p.aoff, p.d_in, p.h1, p.h2, p.d_out, t->work + p.w_ah1, t->work + p.w_ah2, t->work + p.w_amu};
}
static Td3Net td3_critic_net(const ev2g_td3 *t, const float *params, float *out) {
    const Td3Plan &p = t->plan;
    return {params + p.n_actor, p.n_critic, p.coff, p.da, p.h1, p.h2, 1, t->work + p.w_ch1, t->work + p.w_ch2, out};
}

static int td3_launch_refresh(ev2g_handle *h, ev2g_td3 *t) {
    hipLaunchKernelGGL(ev2g_td3_refresh_kernel, dim3(td3_blocks((long long)t->plan.h1 * std::max(t->plan.d_in, t->plan.h2))), dim3(256), 0, h->stream, t->map,
                       (const float *)t->theta);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_td3_default_config(int ddpg, ev2g_td3_config *cfg) {
    if (!cfg) return fail(nullptr, EV2G_ERR_ARG, "ev2g_td3_default_config: cfg is null");
    td3_default_config(ddpg, cfg);
    return EV2G_OK;
}

static int td3_device_stage(ev2g_handle *h, ev2g_td3 *t, ev2g_mlp *m, const float *const *actor, const float *const *critics) {
    const Td3Plan &p = t->plan;
    const size_t G = (size_t)p.n_params;
    float **bufs[] = {&t->theta, &t->target, &t->m, &t->v, &t->grad};
    for (float **b : bufs)
        if (int rc = dalloc(h, t->allocs, G, b)) return rc;
    if (int rc = dalloc(h, t->allocs, (size_t)p.w_floats, &t->work)) return rc;
    if (int rc = dalloc(h, t->allocs, 2, &t->loss)) return rc;
    std::vector<float> host(G);
    for (int i = 0; i < 6; i++) std::copy(actor[i], actor[i] + (p.aoff[i + 1] - p.aoff[i]), host.begin() + p.aoff[i]);
    for (int j = 0; j < p.nc; j++)
        for (int i = 0; i < 6; i++) std::copy(critics[6 * j + i], critics[6 * j + i] + (p.coff[i + 1] - p.coff[i]), host.begin() + p.n_actor + (size_t)j * p.n_critic + p.coff[i]);
    HIPCHK(h, hipMemcpyAsync(t->theta, host.data(), G * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(t->target, t->theta, G * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    const MlpDev &d = m->dev;
    void *const w[3] = {(void *)d.w1, (void *)d.w2, (void *)d.w3};
    float *const b[3] = {(float *)d.b1, (float *)d.b2, (float *)d.b3};
    t->map = mlp_image_map(m->plan, w, b);
    if (int rc = td3_launch_refresh(h, t)) return rc;   // the policy's images from the masters: the two agree by construction
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

int ev2g_td3_create(ev2g_handle *h, ev2g_mlp *policy, const ev2g_td3_config *cfg, int d_in, int h1, int h2, int d_out, const float *const *actor,
                    const float *const *critics, uint64_t seed, ev2g_td3 **out) {
    const char *who = "ev2g_td3_create";
    if (!h || !out) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    *out = nullptr;
    if (!policy || !cfg || !actor || !critics) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (int rc = fields_check(h, who, td3_fields(*cfg))) return rc;
    const Td3Plan plan = plan_td3(d_in, h1, h2, d_out, cfg->n_critics);
    if (plan.err) return fail(h, plan.err, plan.refusal);
    const MlpDev &d = policy->dev;
    const int want[4] = {d.d_in, d.h1, d.h2, d.d_out}, got[4] = {d_in, h1, h2, d_out};
    const char *name[4] = {"d_in", "h1", "h2", "d_out"};
    for (int i = 0; i < 4; i++)
        if (want[i] != got[i])
            return fail(h, EV2G_ERR_ARG, std::string(who) + ": " + name[i] + " " + std::to_string(got[i]) + " is not the policy's " + std::to_string(want[i]));
    for (int i = 0; i < 6 * (1 + cfg->n_critics); i++)
        if (!(i < 6 ? actor[i] : critics[i - 6])) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null weight array");
    if (policy->learner) return fail(h, EV2G_ERR_STATE, std::string(who) + ": the policy already has a learner");
    (void)hipSetDevice(h->device);
    ev2g_td3 *t = new ev2g_td3();
    t->cfg = *cfg; t->plan = plan; t->lo = d.out_lo; t->seed = seed;
    const int rc = owned_created(h, &ev2g_handle::td3s, t, td3_device_stage(h, t, policy, actor, critics), out);
    if (!rc) { t->policy = policy; policy->learner = t; }
    return rc;
}

void ev2g_td3_destroy(ev2g_handle *h, ev2g_td3 *t) { owned_destroy(h, &ev2g_handle::td3s, t, td3_free); }

static int td3_critic_stage(ev2g_handle *h, ev2g_td3 *t, const char *who, const float *obs, const float *actions, const float *reward, const float *next_obs,
                            const uint8_t *done, int B, float *losses) {
    if (int rc = td3_check(h, t, who)) return rc;
    if (!obs || !actions || !reward || !next_obs || !done) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    const std::string refusal = td3_batch_refusal(who, B);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    const Td3Plan &p = t->plan;
    float *W = t->work, *L = losses ? losses : t->loss;
    const float sigma = (float)t->cfg.target_policy_noise, clip = (float)t->cfg.target_noise_clip;
    const unsigned nb = td3_blocks((long long)B * p.da);
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(nb), dim3(256), 0, h->stream, obs, actions, B, p.d_in, p.d_out, t->lo, W + p.w_xa);
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(nb), dim3(256), 0, h->stream, next_obs, (const float *)nullptr, B, p.d_in, p.d_out, t->lo, W + p.w_xb);
    td3_forward(h, td3_actor_net(t, t->target), next_obs, B, TD3_EPI_BIAS_TANH, 1);
    hipLaunchKernelGGL(ev2g_td3_action_cols_kernel<true>, dim3(td3_blocks((long long)B * p.d_out)), dim3(256), 0, h->stream, (const float *)(W + p.w_amu), B, p.d_in,
                       p.d_out, sigma, clip, (uint64_t)t->seed, (uint64_t)t->next_draw, W + p.w_xb);
    if (sigma > 0.0f) t->next_draw += (unsigned long long)B * (unsigned long long)p.d_out;
    td3_forward(h, td3_critic_net(t, t->target, W + p.w_tq), W + p.w_xb, B, TD3_EPI_BIAS, p.nc);
    const Td3Net cn = td3_critic_net(t, t->theta, W + p.w_q);
    td3_forward(h, cn, W + p.w_xa, B, TD3_EPI_BIAS, p.nc);
    hipLaunchKernelGGL(ev2g_td3_critic_head_kernel, dim3(1), dim3(256), 0, h->stream, (const float *)(W + p.w_tq), (const float *)(W + p.w_q), reward, done, B, p.nc,
                       (float)t->cfg.gamma, W + p.w_y, W + p.w_dq, L);
    td3_backward(h, cn, W + p.w_xa, B, W + p.w_dq, W + p.w_d2, W + p.w_d1, t->grad + p.n_actor, nullptr, 0, 0, p.nc);
    HIPCHK(h, hipGetLastError());
    t->pending |= 1; t->last_B = B;
    return EV2G_OK;
}

static int td3_actor_stage(ev2g_handle *h, ev2g_td3 *t, const char *who, const float *obs, int B, float *losses) {
    if (int rc = td3_check(h, t, who)) return rc;
    if (!obs) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    const std::string refusal = td3_batch_refusal(who, B);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    const Td3Plan &p = t->plan;
    float *W = t->work, *L = losses ? losses : t->loss;
    const Td3Net an = td3_actor_net(t, t->theta);
    td3_forward(h, an, obs, B, TD3_EPI_BIAS_TANH, 1);
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(td3_blocks((long long)B * p.da)), dim3(256), 0, h->stream, obs, (const float *)nullptr, B, p.d_in, p.d_out, t->lo,
                       W + p.w_xb);
    hipLaunchKernelGGL(ev2g_td3_action_cols_kernel<false>, dim3(td3_blocks((long long)B * p.d_out)), dim3(256), 0, h->stream, (const float *)(W + p.w_amu), B, p.d_in,
                       p.d_out, 0.0f, 0.0f, (uint64_t)0, (uint64_t)0, W + p.w_xb);
    const Td3Net c0 = td3_critic_net(t, t->theta, W + p.w_q);
    td3_forward(h, c0, W + p.w_xb, B, TD3_EPI_BIAS, 1);
    hipLaunchKernelGGL(ev2g_td3_actor_head_kernel, dim3(1), dim3(256), 0, h->stream, (const float *)(W + p.w_q), B, W + p.w_dq, L);
    td3_backward(h, c0, W + p.w_xb, B, W + p.w_dq, W + p.w_d2, W + p.w_d1, nullptr, W + p.w_dmu, p.d_in, p.d_out, 1);
    hipLaunchKernelGGL(ev2g_td3_tanh_back_kernel, dim3(td3_blocks((long long)B * p.d_out)), dim3(256), 0, h->stream, W + p.w_dmu, (const float *)(W + p.w_amu),
                       (long long)B * p.d_out);
    td3_backward(h, an, obs, B, W + p.w_dmu, W + p.w_e2, W + p.w_e1, t->grad, nullptr, 0, 0, 1);
    HIPCHK(h, hipGetLastError());
    t->pending |= 2;
    return EV2G_OK;
}

static int td3_apply_stage(ev2g_handle *h, ev2g_td3 *t, const char *who) {
    if (int rc = td3_check(h, t, who)) return rc;
    if (!t->pending) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no gradient to apply (ev2g_td3_critic_grad or ev2g_td3_actor_grad first)");
    const Td3Plan &p = t->plan;
    const ev2g_td3_config &c = t->cfg;
    if (t->pending & 1) {
        const long long n = (long long)p.nc * p.n_critic;
        t->t_critic += 1; t->n += 1;
        hipLaunchKernelGGL(ev2g_td3_adam_kernel, dim3(td3_blocks(n)), dim3(256), 0, h->stream, t->theta + p.n_actor, t->m + p.n_actor, t->v + p.n_actor,
                           (const float *)(t->grad + p.n_actor), n, adam_step(c.lr, c.beta1, c.beta2, c.adam_eps, t->t_critic));
    }
    if (t->pending & 2) {
        t->t_actor += 1;
        hipLaunchKernelGGL(ev2g_td3_adam_kernel, dim3(td3_blocks(p.n_actor)), dim3(256), 0, h->stream, t->theta, t->m, t->v, (const float *)t->grad, (long long)p.n_actor,
                           adam_step(c.lr, c.beta1, c.beta2, c.adam_eps, t->t_actor));
        hipLaunchKernelGGL(ev2g_td3_polyak_kernel, dim3(td3_blocks(p.n_params)), dim3(256), 0, h->stream, t->target, (const float *)t->theta, (long long)p.n_params,
                           (float)(1.0 - c.tau), (float)c.tau);
        if (int rc = td3_launch_refresh(h, t)) return rc;
    }
    HIPCHK(h, hipGetLastError());
    t->pending = 0;
    return EV2G_OK;
}

int ev2g_td3_critic_grad(ev2g_handle *h, ev2g_td3 *t, const float *obs, const float *actions, const float *reward, const float *next_obs,
                         const uint8_t *done, int B, float *losses) {
    return td3_critic_stage(h, t, "ev2g_td3_critic_grad", obs, actions, reward, next_obs, done, B, losses);
}
int ev2g_td3_actor_grad(ev2g_handle *h, ev2g_td3 *t, const float *obs, int B, float *losses) { return td3_actor_stage(h, t, "ev2g_td3_actor_grad", obs, B, losses); }
int ev2g_td3_apply(ev2g_handle *h, ev2g_td3 *t) { return td3_apply_stage(h, t, "ev2g_td3_apply"); }

int ev2g_td3_update(ev2g_handle *h, ev2g_td3 *t, const float *obs, const float *actions, const float *reward, const float *next_obs,
                    const uint8_t *done, int B, float *losses) {
    const char *who = "ev2g_td3_update";
    if (int rc = td3_critic_stage(h, t, who, obs, actions, reward, next_obs, done, B, losses)) return rc;
    if (int rc = td3_apply_stage(h, t, who)) return rc;
    if (t->n % t->cfg.policy_delay != 0) return EV2G_OK;
    if (int rc = td3_actor_stage(h, t, who, obs, B, losses)) return rc;
    return td3_apply_stage(h, t, who);
}

// a flat buffer in the plan's layout into 6 + 6 n_critics host arrays (null entries skipped)
static int td3_read_flat(ev2g_handle *h, const Td3Plan &p, const float *src, float *const *out) {
    for (int i = 0; i < 6; i++)
        if (out[i]) HIPCHK(h, hipMemcpyAsync(out[i], src + p.aoff[i], (size_t)(p.aoff[i + 1] - p.aoff[i]) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    for (int j = 0; j < p.nc; j++)
        for (int i = 0; i < 6; i++)
            if (out[6 + 6 * j + i])
                HIPCHK(h, hipMemcpyAsync(out[6 + 6 * j + i], src + p.n_actor + (size_t)j * p.n_critic + p.coff[i], (size_t)(p.coff[i + 1] - p.coff[i]) * sizeof(float),
                                         hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
int ev2g_td3_get_grads(ev2g_handle *h, ev2g_td3 *t, float *const *out) {
    if (int rc = td3_check(h, t, "ev2g_td3_get_grads")) return rc;
    if (!out) return fail(h, EV2G_ERR_ARG, "ev2g_td3_get_grads: null argument");
    return td3_read_flat(h, t->plan, t->grad, out);
}
int ev2g_td3_get_weights(ev2g_handle *h, ev2g_td3 *t, int target, float *const *out) {
    if (int rc = td3_check(h, t, "ev2g_td3_get_weights")) return rc;
    if (!out) return fail(h, EV2G_ERR_ARG, "ev2g_td3_get_weights: null argument");
    return td3_read_flat(h, t->plan, target ? t->target : t->theta, out);
}
int ev2g_td3_get_y(ev2g_handle *h, ev2g_td3 *t, float *y, int B) {
    if (int rc = td3_check(h, t, "ev2g_td3_get_y")) return rc;
    if (!y) return fail(h, EV2G_ERR_ARG, "ev2g_td3_get_y: null argument");
    if (B < 1 || B != t->last_B) return fail(h, EV2G_ERR_ARG, "ev2g_td3_get_y: B is not the batch size of the last critic gradient");
    HIPCHK(h, hipMemcpyAsync(y, t->work + t->plan.w_y, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
int ev2g_td3_set_rate(ev2g_handle *h, ev2g_td3 *t, double lr) {
    if (int rc = td3_check(h, t, "ev2g_td3_set_rate")) return rc;
    if (int rc = fields_check(h, "ev2g_td3_set_rate", td3_rate_fields(lr))) return rc;
    t->cfg.lr = lr;
    return EV2G_OK;
}
int ev2g_td3_seed(ev2g_handle *h, ev2g_td3 *t, uint64_t seed, uint64_t first_draw) {
    if (int rc = td3_check(h, t, "ev2g_td3_seed")) return rc;
    t->seed = seed; t->next_draw = first_draw;
    return EV2G_OK;
}
int ev2g_td3_counters(ev2g_handle *h, ev2g_td3 *t, int64_t *updates, int64_t *actor_steps, uint64_t *next_draw) {
    if (int rc = td3_check(h, t, "ev2g_td3_counters")) return rc;
    if (updates) *updates = t->n;
    if (actor_steps) *actor_steps = t->t_actor;
    if (next_draw) *next_draw = t->next_draw;
    return EV2G_OK;
}

static int replay_args(ev2g_handle *h, const char *who, int B, int n_blocks, int T, int E) {
    const std::string refusal = td3_batch_refusal(who, B);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    if (n_blocks < 1 || n_blocks > EV2G_REPLAY_MAX_BLOCKS) return fail(h, EV2G_ERR_ARG, std::string(who) + ": n_blocks must be 1 .. " + std::to_string(EV2G_REPLAY_MAX_BLOCKS));
    if (T < 1 || E < 1) return fail(h, EV2G_ERR_ARG, std::string(who) + ": T and E must be positive");
    return EV2G_OK;
}
int ev2g_replay_sample(ev2g_handle *h, const ev2g_replay_ring *ring, int B, uint64_t seed, uint64_t counter, float *obs, float *actions, float *reward,
                       float *next_obs, uint8_t *done, int32_t *index) {
    const char *who = "ev2g_replay_sample";
    if (!h || !ring || !ring->obs || !ring->actions || !ring->reward || !ring->done || !obs || !actions || !reward || !next_obs || !done)
        return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (int rc = replay_args(h, who, B, ring->n_blocks, ring->T, ring->E)) return rc;
    if (ring->D < 1 || ring->P < 1) return fail(h, EV2G_ERR_ARG, std::string(who) + ": D and P must be positive");
    ReplayTable tb{};
    for (int i = 0; i < ring->n_blocks; i++) {
        if (!ring->obs[i] || !ring->actions[i] || !ring->reward[i] || !ring->done[i]) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null block pointer");
        tb.obs[i] = ring->obs[i]; tb.actions[i] = ring->actions[i]; tb.reward[i] = ring->reward[i]; tb.done[i] = ring->done[i];
    }
    tb.n = ring->n_blocks; tb.T = ring->T; tb.E = ring->E; tb.D = ring->D; tb.P = ring->P;
    (void)hipSetDevice(h->device);
    hipLaunchKernelGGL(ev2g_replay_sample_kernel, dim3((unsigned)B), dim3(64), 0, h->stream, tb, seed, counter, obs, actions, reward, next_obs, done, (int *)index);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}
int ev2g_host_replay_indices(int32_t *index, int B, int n_blocks, int T, int E, uint64_t seed, uint64_t counter) {
    if (!index) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_replay_indices: null argument");
    if (int rc = replay_args(nullptr, "ev2g_host_replay_indices", B, n_blocks, T, E)) return rc;
    for (int row = 0; row < B; row++) {
        const uint64_t i0 = ev2g_replay_stream_index(counter, row);
        index[3 * row] = ev2g_replay_pick(ev2g_u01(seed, i0), n_blocks);
        index[3 * row + 1] = ev2g_replay_pick(ev2g_u01(seed, i0 + 1), T);
        index[3 * row + 2] = ev2g_replay_pick(ev2g_u01(seed, i0 + 2), E);
    }
    return EV2G_OK;
}

int ev2g_host_td3_target(const float *a_target, const float *tq, const float *reward, const uint8_t *done, int B, int P, int n_critics, double sigma,
                         double clip, double gamma, uint64_t seed, uint64_t first_draw, float *a_next, float *y) {
    const char *who = "ev2g_host_td3_target";
    if (B < 1 || P < 1 || n_critics < 1 || n_critics > 2) return fail(nullptr, EV2G_ERR_ARG, std::string(who) + ": B and P must be positive, n_critics 1 or 2");
    if (!(sigma >= 0.0) || !(clip >= 0.0) || !std::isfinite(sigma) || !std::isfinite(clip))
        return fail(nullptr, EV2G_ERR_ARG, std::string(who) + ": sigma and clip must be finite and >= 0");
    if (a_target && a_next) {
        std::vector<float> normals((size_t)B * P, 0.0f);
        if (sigma > 0.0) ev2g_ac_host_normal(normals.data(), (int64_t)B * P, seed, first_draw);
        td3_host_smooth(a_target, normals.data(), (long long)B * P, sigma, clip, a_next);
    }
    if (tq) {
        if (!reward || !done || !y) return fail(nullptr, EV2G_ERR_ARG, std::string(who) + ": null argument");
        td3_host_y(tq, reward, done, B, n_critics, gamma, y);
    }
    return EV2G_OK;
}
int ev2g_host_polyak(float *target, const float *param, int64_t n, double tau) {
    if (!target || !param || n < 0) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_polyak: null argument or n < 0");
    if (!(tau >= 0.0 && tau <= 1.0)) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_polyak: tau must be in [0, 1]");
    td3_host_polyak(target, param, (long long)n, tau);
    return EV2G_OK;
}

// ---- the SAC learner and its collection actor (ev2g_sac.h) ----
static int sac_check(ev2g_handle *h, ev2g_sac *s, const char *who) { return owned_check(h, &ev2g_handle::sacs, s, "SAC learner", who, false); }

// ev2g_sac_act_kernel<SAMPLE>: the kernel (ev2g_sac_create sets its dynamic-LDS attribute) and its launch
struct SacActEntry {
    const void *fn;
    void (*launch)(const LaunchDims &, const SacDev &, const float *x, int n_rows, uint64_t seed, uint64_t draw0, float *act, float *mu, float *ls, float *logp);
};
extern "C++" template <bool SAMPLE>
static void launch_sac_act(const LaunchDims &d, const SacDev &dev, const float *x, int n_rows, uint64_t seed, uint64_t draw0, float *act, float *mu, float *ls,
                           float *logp) {
    hipLaunchKernelGGL(ev2g_sac_act_kernel<SAMPLE>, d.grid, dim3(EV2G_AC_BLOCK), d.lds, d.stream, dev, x, n_rows, seed, draw0, act, mu, ls, logp);
}
static const SacActEntry &sac_act_kernel(bool sample) {
    static const SacActEntry tab[2] = {{(const void *)ev2g_sac_act_kernel<false>, &launch_sac_act<false>}, {(const void *)ev2g_sac_act_kernel<true>, &launch_sac_act<true>}};
    return tab[sample ? 1 : 0];
}

// the actor's trunk and mu head as a Td3Net (the log_std head is the z = 1 block behind mu's: SacPlan::head_block), and the critics
static Td3Net sac_actor_net(const SacCore *s) {
    const SacPlan &p = s->plan;
    return {s->theta, 0, p.aoff, p.d_in, p.h1, p.h2, p.d_out, s->work + p.w_ah1, s->work + p.w_ah2, s->work + p.w_head};
}
static Td3Net sac_critic_net(const SacCore *s, const float *critic_params, float *out) {
    const SacPlan &p = s->plan;
    return {critic_params, p.n_critic, p.coff, p.da, p.h1, p.h2, p.coff[6] - p.coff[5], s->work + p.w_ch1, s->work + p.w_ch2, out};
}

// the actor on x [B, d_in] with the draws draw0 + b P + p: the trunk, both heads (the z dimension of one launch), then the squashed-Gaussian
// head: mu | raw log_std, eps and a into the workspace, a into the action columns of xcols [B, da], log pi into logp
static void sac_actor_forward(ev2g_handle *h, SacCore *s, const float *x, int B, uint64_t draw0, float *xcols, float *logp) {
    const SacPlan &p = s->plan;
    float *W = s->work;
    const Td3Net an = sac_actor_net(s);
    const long long z1 = (long long)B * p.h1, z2 = (long long)B * p.h2;
    Td3Gemm g{};
    g.M = B; g.sak = 1; g.sbk = 1;
    g.A = x; g.sam = p.d_in; g.K = p.d_in; g.N = p.h1; g.Bm = an.th + p.aoff[0]; g.sbn = p.d_in; g.bias = an.th + p.aoff[1]; g.C = an.H1; g.ldc = p.h1; g.zC = z1;
    g.epi = TD3_EPI_BIAS_RELU;
    td3_gemm(h, g, 1);
    g.A = an.H1; g.sam = p.h1; g.K = p.h1; g.N = p.h2; g.Bm = an.th + p.aoff[2]; g.sbn = p.h1; g.bias = an.th + p.aoff[3]; g.C = an.H2; g.ldc = p.h2; g.zC = z2;
    td3_gemm(h, g, 1);
    g.A = an.H2; g.zA = 0; g.sam = p.h2; g.K = p.h2; g.N = p.d_out; g.Bm = an.th + p.aoff[4]; g.zB = p.head_block; g.sbn = p.h2; g.bias = an.th + p.aoff[5];
    g.zbias = p.head_block; g.C = W + p.w_head; g.ldc = p.d_out; g.zC = (long long)B * p.d_out; g.epi = TD3_EPI_BIAS;
    td3_gemm(h, g, 2);
    hipLaunchKernelGGL(ev2g_sac_head_kernel, dim3((unsigned)((B + 31) / 32)), dim3(256), 0, h->stream, (const float *)(W + p.w_head),
                       (const float *)(W + p.w_head + (long long)B * p.d_out), B, p.d_out, (uint64_t)s->seed, draw0, W + p.w_eps, W + p.w_a, xcols, p.da, p.d_in, logp);
}

static int sac_launch_repack(ev2g_handle *h, SacCore *s) {
    SacRepack r{};
    for (int i = 0; i <= EV2G_SAC_ACTOR_ARRAYS; i++) r.off[i] = s->plan.aoff[i];
    hipLaunchKernelGGL(ev2g_sac_repack_kernel, dim3(td3_blocks((long long)s->plan.h1 * std::max(s->plan.d_in, s->plan.h2))), dim3(256), 0, h->stream, s->dev, r,
                       (const float *)s->theta);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_sac_default_config(ev2g_sac_config *cfg) {
    if (!cfg) return fail(nullptr, EV2G_ERR_ARG, "ev2g_sac_default_config: cfg is null");
    sac_default_config(cfg);
    return EV2G_OK;
}

static int sac_device_stage(ev2g_handle *h, SacCore *s, const float *const *actor, const float *const *critics) {
    const SacPlan &p = s->plan;
    const size_t G = (size_t)p.n_params, GC = (size_t)p.nc * p.n_critic;
    float **bufs[] = {&s->theta, &s->m, &s->v, &s->grad};
    for (float **b : bufs)
        if (int rc = dalloc(h, s->allocs, G, b)) return rc;
    if (int rc = dalloc(h, s->allocs, GC, &s->target)) return rc;
    if (int rc = dalloc(h, s->allocs, (size_t)p.w_floats, &s->work)) return rc;
    if (int rc = dalloc(h, s->allocs, 4, &s->loss)) return rc;
    if (int rc = dalloc(h, s->allocs, 3, &s->alpha)) return rc;
    if (int rc = dalloc(h, s->allocs, 1, &s->g_alpha)) return rc;
    size_t img[6];
    sac_image_sizes(p, img);
    float **imgs[6] = {&s->dev.w1, &s->dev.b1, &s->dev.w2, &s->dev.b2, &s->dev.wh, &s->dev.bh};
    for (int i = 0; i < 6; i++)
        if (int rc = dalloc(h, s->allocs, img[i], imgs[i])) return rc;   // (zeros: the padding the repack never writes)
    std::vector<float> host(G);
    for (int i = 0; i < EV2G_SAC_ACTOR_ARRAYS; i++) std::copy(actor[i], actor[i] + (p.aoff[i + 1] - p.aoff[i]), host.begin() + p.aoff[i]);
    for (int j = 0; j < p.nc; j++)
        for (int i = 0; i < 6; i++) std::copy(critics[6 * j + i], critics[6 * j + i] + (p.coff[i + 1] - p.coff[i]), host.begin() + p.n_actor + (size_t)j * p.n_critic + p.coff[i]);
    const float la = (float)std::log(s->cfg.ent_coef);
    HIPCHK(h, hipMemcpyAsync(s->theta, host.data(), G * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->target, s->theta + p.n_actor, GC * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->alpha, &la, sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (int rc = sac_launch_repack(h, s)) return rc;
    for (unsigned k = 0; k < 2; k++)
        if (s->lds > 48 * 1024 && !(h->sac_attr_mask & (1u << k))) {   // (function attributes are per device: once per handle, for the largest network)
            const hipError_t e = hipFuncSetAttribute(sac_act_kernel(k != 0).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ev2g_sac_lds_max());
            if (e != hipSuccess) return fail(h, EV2G_ERR_HIP, std::string(s->abi) + "_create: hipFuncSetAttribute: " + hipGetErrorString(e));
            h->sac_attr_mask |= 1u << k;
        }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

int ev2g_sac_create(ev2g_handle *h, const ev2g_sac_config *cfg, int d_in, int h1, int h2, int d_out, float lo, const float *const *actor,
                    const float *const *critics, uint64_t seed, ev2g_sac **out) {
    const char *who = "ev2g_sac_create";
    if (!h || !out) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    *out = nullptr;
    if (!cfg || !actor || !critics) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (int rc = fields_check(h, who, sac_fields(*cfg))) return rc;
    const SacPlan plan = plan_sac(d_in, h1, h2, d_out, cfg->n_critics);
    if (plan.err) return fail(h, plan.err, plan.refusal);
    if (lo != -1.0f && lo != 0.0f) return fail(h, EV2G_ERR_ARG, std::string(who) + ": lo must be -1 or 0");
    for (int i = 0; i < EV2G_SAC_ACTOR_ARRAYS + 6 * cfg->n_critics; i++)
        if (!(i < EV2G_SAC_ACTOR_ARRAYS ? actor[i] : critics[i - EV2G_SAC_ACTOR_ARRAYS])) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null weight array");
    (void)hipSetDevice(h->device);
    ev2g_sac *s = new ev2g_sac();
    s->cfg = *cfg; s->plan = plan; s->lo = lo; s->seed = seed; s->act_seed = seed;
    s->target_entropy = sac_target_entropy(*cfg, d_out);
    s->dev = sac_dev(plan, lo);
    s->lds = ev2g_sac_lds(s->dev).bytes;
    const int rc = owned_created(h, &ev2g_handle::sacs, s, sac_device_stage(h, s, actor, critics), out);
    return rc;
}

void ev2g_sac_destroy(ev2g_handle *h, ev2g_sac *s) { owned_destroy(h, &ev2g_handle::sacs, s); }

static int sac_critic_stage(ev2g_handle *h, ev2g_sac *s, const char *who, const float *obs, const float *actions, const float *reward, const float *next_obs,
                            const uint8_t *done, int B, float *losses) {
    if (int rc = sac_check(h, s, who)) return rc;
    if (!obs || !actions || !reward || !next_obs || !done) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    const std::string refusal = td3_batch_refusal(who, B);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    const SacPlan &p = s->plan;
    float *W = s->work, *L = losses ? losses : s->loss;
    const unsigned nb = td3_blocks((long long)B * p.da);
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(nb), dim3(256), 0, h->stream, obs, actions, B, p.d_in, p.d_out, s->lo, W + p.w_xa);
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(nb), dim3(256), 0, h->stream, next_obs, (const float *)nullptr, B, p.d_in, p.d_out, s->lo, W + p.w_xb);
    sac_actor_forward(h, s, next_obs, B, (uint64_t)s->next_draw + (uint64_t)B * (uint64_t)p.d_out, W + p.w_xb, W + p.w_lp2);
    td3_forward(h, sac_critic_net(s, s->target, W + p.w_tq), W + p.w_xb, B, TD3_EPI_BIAS, p.nc);
    const Td3Net cn = sac_critic_net(s, s->theta + p.n_actor, W + p.w_q);
    td3_forward(h, cn, W + p.w_xa, B, TD3_EPI_BIAS, p.nc);
    hipLaunchKernelGGL(ev2g_sac_critic_head_kernel, dim3(1), dim3(256), 0, h->stream, (const float *)(W + p.w_tq), (const float *)(W + p.w_q),
                       (const float *)(W + p.w_lp2), reward, done, B, p.nc, s->cfg.gamma, (const float *)s->alpha, W + p.w_y, W + p.w_dq, L);
    td3_backward(h, cn, W + p.w_xa, B, W + p.w_dq, W + p.w_d2, W + p.w_d1, s->grad + p.n_actor, nullptr, 0, 0, p.nc);
    HIPCHK(h, hipGetLastError());
    s->pending |= 1; s->last_B = B;
    return EV2G_OK;
}

// The actor's backward from the input-delta blocks dxa [nc][B, P] that ev2g_sac_head_back_kernel sums -- SAC passes its critics' blocks (nc 1 or
// 2: the kernel's limit), TQC always ONE block, its up to five critics' deltas already summed by ev2g_tqc_delta_sum_kernel -- of the forward
// sac_actor_forward left in the workspace: the eight gradients into grad
static void sac_actor_backward(ev2g_handle *h, SacCore *s, const float *obs, int B, const float *dxa, int nc) {
    const SacPlan &p = s->plan;
    float *W = s->work;
    const long long BP = (long long)B * p.d_out, z2 = (long long)B * p.h2;
    hipLaunchKernelGGL(ev2g_sac_head_back_kernel, dim3(td3_blocks(BP)), dim3(256), 0, h->stream, (const float *)(W + p.w_head), (const float *)(W + p.w_head + BP),
                       (const float *)(W + p.w_eps), dxa, nc, B, p.d_out, (const float *)s->alpha, W + p.w_dhead);
    // the heads (z = 0: mu, 1: log_std): their gradients, their backward-data products joined under the second hidden layer's ReLU, then the trunk
    const Td3Net an = sac_actor_net(s);
    td3_wgrad(h, B, W + p.w_dhead, BP, p.d_out, an.H2, 0, p.h2, s->grad + p.aoff[4], s->grad + p.aoff[5], p.head_block, 2);
    td3_bdata(h, B, W + p.w_dhead, BP, p.d_out, s->theta + p.aoff[4], p.head_block, p.h2, p.h2, nullptr, 0, W + p.w_e2z, z2, 2);
    hipLaunchKernelGGL(ev2g_sac_join_kernel, dim3(td3_blocks(z2)), dim3(256), 0, h->stream, (const float *)(W + p.w_e2z), (const float *)(W + p.w_e2z + z2),
                       (const float *)an.H2, z2, W + p.w_e2);
    td3_wgrad(h, B, W + p.w_e2, z2, p.h2, an.H1, 0, p.h1, s->grad + p.aoff[2], s->grad + p.aoff[3], 0, 1);
    td3_bdata(h, B, W + p.w_e2, z2, p.h2, s->theta + p.aoff[2], 0, p.h1, p.h1, an.H1, 0, W + p.w_e1, 0, 1);
    td3_wgrad(h, B, W + p.w_e1, 0, p.h1, obs, 0, p.d_in, s->grad + p.aoff[0], s->grad + p.aoff[1], 0, 1);
}

static int sac_actor_stage(ev2g_handle *h, ev2g_sac *s, const char *who, const float *obs, int B, float *losses) {
    if (int rc = sac_check(h, s, who)) return rc;
    if (!obs) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    const std::string refusal = td3_batch_refusal(who, B);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    const SacPlan &p = s->plan;
    float *W = s->work, *L = losses ? losses : s->loss;
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(td3_blocks((long long)B * p.da)), dim3(256), 0, h->stream, obs, (const float *)nullptr, B, p.d_in, p.d_out, s->lo,
                       W + p.w_xb);
    sac_actor_forward(h, s, obs, B, (uint64_t)s->next_draw, W + p.w_xb, W + p.w_lp);
    const Td3Net cn = sac_critic_net(s, s->theta + p.n_actor, W + p.w_q);
    td3_forward(h, cn, W + p.w_xb, B, TD3_EPI_BIAS, p.nc);
    hipLaunchKernelGGL(ev2g_sac_actor_head_kernel, dim3(1), dim3(256), 0, h->stream, (const float *)(W + p.w_q), (const float *)(W + p.w_lp), B, p.nc,
                       (const float *)s->alpha, s->target_entropy, s->cfg.ent_coef_auto ? 1 : 0, W + p.w_dq, L, s->g_alpha);
    // dQ_j / da of both critics from the selector as output delta: the critic that is not a row's argmin propagates exact zeros
    td3_backward(h, cn, W + p.w_xb, B, W + p.w_dq, W + p.w_d2, W + p.w_d1, nullptr, W + p.w_dxa, p.d_in, p.d_out, p.nc);
    sac_actor_backward(h, s, obs, B, W + p.w_dxa, p.nc);
    HIPCHK(h, hipGetLastError());
    s->pending |= 2; s->last_actor_B = B;
    return EV2G_OK;
}

// (the caller has checked the object)
static int sac_apply_stage(ev2g_handle *h, SacCore *s, const char *who) {
    if (!s->pending) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no gradient to apply (" + s->abi + "_critic_grad or " + s->abi + "_actor_grad first)");
    const SacPlan &p = s->plan;
    const ev2g_sac_config &c = s->cfg;
    if (s->pending & 1) {
        const long long n = (long long)p.nc * p.n_critic;
        s->t_critic += 1;
        hipLaunchKernelGGL(ev2g_td3_adam_kernel, dim3(td3_blocks(n)), dim3(256), 0, h->stream, s->theta + p.n_actor, s->m + p.n_actor, s->v + p.n_actor,
                           (const float *)(s->grad + p.n_actor), n, adam_step(c.lr, c.beta1, c.beta2, c.adam_eps, s->t_critic));
    }
    if (s->pending & 2) {
        s->t_actor += 1; s->n += 1;
        const AdamStep a = adam_step(c.lr, c.beta1, c.beta2, c.adam_eps, s->t_actor);
        hipLaunchKernelGGL(ev2g_td3_adam_kernel, dim3(td3_blocks(p.n_actor)), dim3(256), 0, h->stream, s->theta, s->m, s->v, (const float *)s->grad, (long long)p.n_actor, a);
        if (c.ent_coef_auto) hipLaunchKernelGGL(ev2g_sac_alpha_adam_kernel, dim3(1), dim3(64), 0, h->stream, s->alpha, (const float *)s->g_alpha, a);
        if (s->n % c.target_update_interval == 0) {
            const long long n = (long long)p.nc * p.n_critic;
            s->n_target += 1;
            hipLaunchKernelGGL(ev2g_td3_polyak_kernel, dim3(td3_blocks(n)), dim3(256), 0, h->stream, s->target, (const float *)(s->theta + p.n_actor), n,
                               (float)(1.0 - c.tau), (float)c.tau);
        }
        s->next_draw += 2ull * (unsigned long long)s->last_actor_B * (unsigned long long)p.d_out;
        if (int rc = sac_launch_repack(h, s)) return rc;
    }
    HIPCHK(h, hipGetLastError());
    s->pending = 0;
    return EV2G_OK;
}

int ev2g_sac_critic_grad(ev2g_handle *h, ev2g_sac *s, const float *obs, const float *actions, const float *reward, const float *next_obs,
                         const uint8_t *done, int B, float *losses) {
    return sac_critic_stage(h, s, "ev2g_sac_critic_grad", obs, actions, reward, next_obs, done, B, losses);
}
int ev2g_sac_actor_grad(ev2g_handle *h, ev2g_sac *s, const float *obs, int B, float *losses) { return sac_actor_stage(h, s, "ev2g_sac_actor_grad", obs, B, losses); }
int ev2g_sac_apply(ev2g_handle *h, ev2g_sac *s) {
    if (int rc = sac_check(h, s, "ev2g_sac_apply")) return rc;
    return sac_apply_stage(h, s, "ev2g_sac_apply");
}

int ev2g_sac_update(ev2g_handle *h, ev2g_sac *s, const float *obs, const float *actions, const float *reward, const float *next_obs,
                    const uint8_t *done, int B, float *losses) {
    const char *who = "ev2g_sac_update";
    if (int rc = sac_critic_stage(h, s, who, obs, actions, reward, next_obs, done, B, losses)) return rc;
    if (int rc = sac_apply_stage(h, s, who)) return rc;
    if (int rc = sac_actor_stage(h, s, who, obs, B, losses)) return rc;
    return sac_apply_stage(h, s, who);
}

// one launch of ev2g_sac_act_kernel over n_rows rows; a sampling launch takes the collection stream's counter and advances it
static int sac_act_launch(ev2g_handle *h, SacCore *s, const float *x, int n_rows, bool sample, float *act, float *mu, float *ls, float *logp) {
    const LaunchDims dims{dim3((unsigned)((n_rows + EV2G_AC_ROWS - 1) / EV2G_AC_ROWS)), s->lds, h->stream};
    sac_act_kernel(sample).launch(dims, s->dev, x, n_rows, (uint64_t)s->act_seed, (uint64_t)s->act_n * (uint64_t)n_rows, act, mu, ls, logp);
    HIPCHK(h, hipGetLastError());
    if (sample) s->act_n += 1;
    return EV2G_OK;
}

// ---- the entries SAC and TQC share, behind each object's own check (`who`: the entry's name) ----
static int core_act(ev2g_handle *h, SacCore *s, const char *who, const float *obs32, int n_rows, int deterministic, float *actions, float *mu, float *log_std,
                    float *log_pi) {
    if (!obs32 || !actions || n_rows <= 0) return fail(h, EV2G_ERR_ARG, std::string(who) + ": obs32 or actions is null, or n_rows is not positive");
    return sac_act_launch(h, s, obs32, n_rows, !deterministic, actions, mu, log_std, log_pi);
}
static int core_collect(ev2g_handle *h, SacCore *s, const char *who, int k_steps, int deterministic, const ev2g_transitions *tr) {
    if (!h->loaded) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no scenarios loaded");
    if (s->plan.d_in != h->D || s->plan.d_out != h->P) return fail(h, EV2G_ERR_ARG, std::string(who) + ": actor shape != (obs dim, ports)");
    return collect_rows(h, who, k_steps, tr, nullptr,
                        [&](const float *obs, float *act, int n) { return sac_act_launch(h, s, obs, n, !deterministic, act, nullptr, nullptr, nullptr); });
}
// a flat buffer in the plan's layout into 8 + 6 n_critics host arrays (null entries skipped); actor_src null: the actor's entries are not written
static int sac_read_flat(ev2g_handle *h, const SacPlan &p, const float *actor_src, const float *critic_src, float *const *out) {
    for (int i = 0; i < EV2G_SAC_ACTOR_ARRAYS; i++)
        if (actor_src && out[i]) HIPCHK(h, hipMemcpyAsync(out[i], actor_src + p.aoff[i], (size_t)(p.aoff[i + 1] - p.aoff[i]) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    for (int j = 0; j < p.nc; j++)
        for (int i = 0; i < 6; i++)
            if (float *dst = out[EV2G_SAC_ACTOR_ARRAYS + 6 * j + i])
                HIPCHK(h, hipMemcpyAsync(dst, critic_src + (size_t)j * p.n_critic + p.coff[i], (size_t)(p.coff[i + 1] - p.coff[i]) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
static int core_get_grads(ev2g_handle *h, SacCore *s, const char *who, float *const *out, float *g_log_ent_coef) {
    if (!out) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (g_log_ent_coef) HIPCHK(h, hipMemcpyAsync(g_log_ent_coef, s->g_alpha, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return sac_read_flat(h, s->plan, s->grad, s->grad + s->plan.n_actor, out);
}
static int core_get_weights(ev2g_handle *h, SacCore *s, const char *who, int target, float *const *out) {
    if (!out) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    return target ? sac_read_flat(h, s->plan, nullptr, s->target, out) : sac_read_flat(h, s->plan, s->theta, s->theta + s->plan.n_actor, out);
}
// n floats per row of the last gradient of a half (dst), and one per row (dst2, may be null)
static int sac_read_rows(ev2g_handle *h, const char *who, float *dst, const float *src, float *dst2, const float *src2, int B, int want_B, int n = 1) {
    if (!dst) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (B < 1 || B != want_B) return fail(h, EV2G_ERR_ARG, std::string(who) + ": B is not the batch size of the last gradient of that half");
    HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)B * n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (dst2) HIPCHK(h, hipMemcpyAsync(dst2, src2, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
static int core_get_ent_coef(ev2g_handle *h, SacCore *s, const char *who, float *out3) {
    if (!out3) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    HIPCHK(h, hipMemcpyAsync(out3, s->alpha, 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
static int core_set_rate(ev2g_handle *h, SacCore *s, const char *who, double lr) {
    if (int rc = fields_check(h, who, sac_rate_fields(lr))) return rc;
    s->cfg.lr = lr;
    return EV2G_OK;
}
static int core_counters(SacCore *s, int64_t *updates, int64_t *target_updates, uint64_t *next_draw, uint64_t *act_launches) {
    if (updates) *updates = s->n;
    if (target_updates) *target_updates = s->n_target;
    if (next_draw) *next_draw = s->next_draw;
    if (act_launches) *act_launches = s->act_n;
    return EV2G_OK;
}

int ev2g_sac_act(ev2g_handle *h, ev2g_sac *s, const float *obs32, int n_rows, int deterministic, float *actions, float *mu, float *log_std, float *log_pi) {
    if (int rc = sac_check(h, s, "ev2g_sac_act")) return rc;
    return core_act(h, s, "ev2g_sac_act", obs32, n_rows, deterministic, actions, mu, log_std, log_pi);
}
int ev2g_sac_collect(ev2g_handle *h, ev2g_sac *s, int k_steps, int deterministic, const ev2g_transitions *tr) {
    if (int rc = sac_check(h, s, "ev2g_sac_collect")) return rc;
    return core_collect(h, s, "ev2g_sac_collect", k_steps, deterministic, tr);
}
int ev2g_sac_get_grads(ev2g_handle *h, ev2g_sac *s, float *const *out, float *g_log_ent_coef) {
    if (int rc = sac_check(h, s, "ev2g_sac_get_grads")) return rc;
    return core_get_grads(h, s, "ev2g_sac_get_grads", out, g_log_ent_coef);
}
int ev2g_sac_get_weights(ev2g_handle *h, ev2g_sac *s, int target, float *const *out) {
    if (int rc = sac_check(h, s, "ev2g_sac_get_weights")) return rc;
    return core_get_weights(h, s, "ev2g_sac_get_weights", target, out);
}
int ev2g_sac_get_y(ev2g_handle *h, ev2g_sac *s, float *y, float *log_pi_next, int B) {
    if (int rc = sac_check(h, s, "ev2g_sac_get_y")) return rc;
    return sac_read_rows(h, "ev2g_sac_get_y", y, s->work + s->plan.w_y, log_pi_next, s->work + s->plan.w_lp2, B, s->last_B);
}
int ev2g_sac_get_log_pi(ev2g_handle *h, ev2g_sac *s, float *log_pi, int B) {
    if (int rc = sac_check(h, s, "ev2g_sac_get_log_pi")) return rc;
    return sac_read_rows(h, "ev2g_sac_get_log_pi", log_pi, s->work + s->plan.w_lp, nullptr, nullptr, B, s->last_actor_B);
}
int ev2g_sac_get_ent_coef(ev2g_handle *h, ev2g_sac *s, float *out3) {
    if (int rc = sac_check(h, s, "ev2g_sac_get_ent_coef")) return rc;
    return core_get_ent_coef(h, s, "ev2g_sac_get_ent_coef", out3);
}
int ev2g_sac_set_rate(ev2g_handle *h, ev2g_sac *s, double lr) {
    if (int rc = sac_check(h, s, "ev2g_sac_set_rate")) return rc;
    return core_set_rate(h, s, "ev2g_sac_set_rate", lr);
}
int ev2g_sac_seed(ev2g_handle *h, ev2g_sac *s, uint64_t seed, uint64_t first_draw) {
    if (int rc = sac_check(h, s, "ev2g_sac_seed")) return rc;
    s->seed = seed; s->next_draw = first_draw;
    return EV2G_OK;
}
int ev2g_sac_act_seed(ev2g_handle *h, ev2g_sac *s, uint64_t seed, uint64_t first_launch) {
    if (int rc = sac_check(h, s, "ev2g_sac_act_seed")) return rc;
    s->act_seed = seed; s->act_n = first_launch;
    return EV2G_OK;
}
int ev2g_sac_counters(ev2g_handle *h, ev2g_sac *s, int64_t *updates, int64_t *target_updates, uint64_t *next_draw, uint64_t *act_launches) {
    if (int rc = sac_check(h, s, "ev2g_sac_counters")) return rc;
    return core_counters(s, updates, target_updates, next_draw, act_launches);
}

int ev2g_host_sac_head(const float *mu, const float *log_std, const float *eps, int B, int P, float lo, float *a, float *a_env, float *log_pi) {
    if (!mu || !log_std || !eps || !a || !log_pi) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_sac_head: null argument");
    if (B < 1 || P < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_sac_head: B and P must be positive");
    sac_host_head(mu, log_std, eps, B, P, lo, a, a_env, log_pi);
    return EV2G_OK;
}
int ev2g_host_sac_head_back(const float *mu, const float *log_std, const float *eps, const float *g, int B, int P, float log_ent_coef, float *d_mu,
                            float *d_log_std) {
    if (!mu || !log_std || !eps || !g || !d_mu || !d_log_std) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_sac_head_back: null argument");
    if (B < 1 || P < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_sac_head_back: B and P must be positive");
    sac_host_head_back(mu, log_std, eps, g, B, P, log_ent_coef, d_mu, d_log_std);
    return EV2G_OK;
}
int ev2g_host_sac_y(const float *tq, const float *log_pi_next, const float *reward, const uint8_t *done, int B, int n_critics, double gamma,
                    float log_ent_coef, float *y) {
    if (!tq || !log_pi_next || !reward || !done || !y) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_sac_y: null argument");
    if (B < 1 || n_critics < 1 || n_critics > 2) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_sac_y: B must be positive, n_critics 1 or 2");
    sac_host_y(tq, log_pi_next, reward, done, B, n_critics, gamma, log_ent_coef, y);
    return EV2G_OK;
}

// ---- the TQC learner and its collection actor (ev2g_tqc.h): SacCore with quantile critics ----
static int tqc_check(ev2g_handle *h, ev2g_tqc *t, const char *who) { return owned_check(h, &ev2g_handle::tqcs, t, "TQC learner", who, false); }

int ev2g_tqc_default_config(ev2g_tqc_config *cfg) {
    if (!cfg) return fail(nullptr, EV2G_ERR_ARG, "ev2g_tqc_default_config: cfg is null");
    tqc_default_config(cfg);
    return EV2G_OK;
}

int ev2g_tqc_create(ev2g_handle *h, const ev2g_tqc_config *cfg, int d_in, int h1, int h2, int d_out, float lo, const float *const *actor,
                    const float *const *critics, uint64_t seed, ev2g_tqc **out) {
    const char *who = "ev2g_tqc_create";
    if (!h || !out) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    *out = nullptr;
    if (!cfg || !actor || !critics) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (int rc = fields_check(h, who, tqc_fields(*cfg))) return rc;
    const TqcPlan plan = plan_tqc(d_in, h1, h2, d_out, cfg->n_critics, cfg->n_quantiles, cfg->top_quantiles_to_drop_per_net);
    if (plan.err) return fail(h, plan.err, plan.refusal);
    if (lo != -1.0f && lo != 0.0f) return fail(h, EV2G_ERR_ARG, std::string(who) + ": lo must be -1 or 0");
    for (int i = 0; i < EV2G_SAC_ACTOR_ARRAYS + 6 * cfg->n_critics; i++)
        if (!(i < EV2G_SAC_ACTOR_ARRAYS ? actor[i] : critics[i - EV2G_SAC_ACTOR_ARRAYS])) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null weight array");
    (void)hipSetDevice(h->device);
    ev2g_tqc *t = new ev2g_tqc();
    t->abi = "ev2g_tqc";
    t->cfg = tqc_sac_config(*cfg); t->tq = plan; t->plan = plan;   // (plan.w_floats: SAC's blocks and TQC's behind them)
    t->lo = lo; t->seed = seed; t->act_seed = seed;
    t->target_entropy = sac_target_entropy(t->cfg, d_out);
    t->dev = sac_dev(plan, lo);
    t->lds = ev2g_sac_lds(t->dev).bytes;
    return owned_created(h, &ev2g_handle::tqcs, t, sac_device_stage(h, t, actor, critics), out);
}

void ev2g_tqc_destroy(ev2g_handle *h, ev2g_tqc *t) { owned_destroy(h, &ev2g_handle::tqcs, t); }

static void tqc_launch_target(ev2g_handle *h, const float *tq, const float *lp, const float *reward, const uint8_t *done, int B, int nc, int nq, int K, double gamma,
                              const float *log_alpha, float *z) {
    hipLaunchKernelGGL(ev2g_tqc_target_kernel, dim3((unsigned)((B + EV2G_TQC_ROWS - 1) / EV2G_TQC_ROWS)), dim3(64 * EV2G_TQC_ROWS), 0, h->stream, tq, lp, reward, done, B, nc,
                       nq, K, gamma, log_alpha, z);
}

static int tqc_critic_stage(ev2g_handle *h, ev2g_tqc *t, const char *who, const float *obs, const float *actions, const float *reward, const float *next_obs,
                            const uint8_t *done, int B, float *losses) {
    if (int rc = tqc_check(h, t, who)) return rc;
    if (!obs || !actions || !reward || !next_obs || !done) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    const std::string refusal = td3_batch_refusal(who, B);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    const TqcPlan &p = t->tq;
    float *W = t->work, *L = losses ? losses : t->loss;
    double *part = (double *)(W + p.w_part);
    const unsigned nb = td3_blocks((long long)B * p.da), rb = (unsigned)((B + EV2G_TQC_ROWS - 1) / EV2G_TQC_ROWS);
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(nb), dim3(256), 0, h->stream, obs, actions, B, p.d_in, p.d_out, t->lo, W + p.w_xa);
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(nb), dim3(256), 0, h->stream, next_obs, (const float *)nullptr, B, p.d_in, p.d_out, t->lo, W + p.w_xb);
    sac_actor_forward(h, t, next_obs, B, (uint64_t)t->next_draw + (uint64_t)B * (uint64_t)p.d_out, W + p.w_xb, W + p.w_lp2);
    td3_forward(h, sac_critic_net(t, t->target, W + p.w_tq), W + p.w_xb, B, TD3_EPI_BIAS, p.nc);
    const Td3Net cn = sac_critic_net(t, t->theta + p.n_actor, W + p.w_q);
    td3_forward(h, cn, W + p.w_xa, B, TD3_EPI_BIAS, p.nc);
    tqc_launch_target(h, W + p.w_tq, W + p.w_lp2, reward, done, B, p.nc, p.nq, p.K, t->cfg.gamma, t->alpha, W + p.w_z);
    hipLaunchKernelGGL(ev2g_tqc_critic_head_kernel, dim3(rb), dim3(64 * EV2G_TQC_ROWS), 0, h->stream, (const float *)(W + p.w_z), (const float *)(W + p.w_q), B, p.nc, p.nq,
                       p.K, W + p.w_dq, part);
    hipLaunchKernelGGL(ev2g_tqc_loss_join_kernel, dim3(1), dim3(256), 0, h->stream, (const double *)part, B, p.nc, p.nq, p.K, L);
    td3_backward(h, cn, W + p.w_xa, B, W + p.w_dq, W + p.w_d2, W + p.w_d1, t->grad + p.n_actor, nullptr, 0, 0, p.nc);
    HIPCHK(h, hipGetLastError());
    t->pending |= 1; t->last_B = B;
    return EV2G_OK;
}

static int tqc_actor_stage(ev2g_handle *h, ev2g_tqc *t, const char *who, const float *obs, int B, float *losses) {
    if (int rc = tqc_check(h, t, who)) return rc;
    if (!obs) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    const std::string refusal = td3_batch_refusal(who, B);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    const TqcPlan &p = t->tq;
    float *W = t->work, *L = losses ? losses : t->loss;
    double *part = (double *)(W + p.w_part);
    const long long BP = (long long)B * p.d_out;
    hipLaunchKernelGGL(ev2g_td3_concat_kernel, dim3(td3_blocks((long long)B * p.da)), dim3(256), 0, h->stream, obs, (const float *)nullptr, B, p.d_in, p.d_out, t->lo,
                       W + p.w_xb);
    sac_actor_forward(h, t, obs, B, (uint64_t)t->next_draw, W + p.w_xb, W + p.w_lp);
    const Td3Net cn = sac_critic_net(t, t->theta + p.n_actor, W + p.w_q);
    td3_forward(h, cn, W + p.w_xb, B, TD3_EPI_BIAS, p.nc);
    hipLaunchKernelGGL(ev2g_tqc_actor_rows_kernel, dim3(td3_blocks((long long)p.nc * B * p.nq)), dim3(256), 0, h->stream, (const float *)(W + p.w_q), B, p.nc, p.nq,
                       W + p.w_dq, part);
    hipLaunchKernelGGL(ev2g_tqc_actor_head_kernel, dim3(1), dim3(256), 0, h->stream, (const double *)part, (const float *)(W + p.w_lp), B, p.nc, p.nq,
                       (const float *)t->alpha, t->target_entropy, t->cfg.ent_coef_auto ? 1 : 0, L, t->g_alpha);
    // d mean_{j,i} q / da: every critic's input delta from the uniform output delta, summed j ascending
    td3_backward(h, cn, W + p.w_xb, B, W + p.w_dq, W + p.w_d2, W + p.w_d1, nullptr, W + p.w_dxa, p.d_in, p.d_out, p.nc);
    hipLaunchKernelGGL(ev2g_tqc_delta_sum_kernel, dim3(td3_blocks(BP)), dim3(256), 0, h->stream, (const float *)(W + p.w_dxa), p.nc, BP, W + p.w_g);
    sac_actor_backward(h, t, obs, B, W + p.w_g, 1);
    HIPCHK(h, hipGetLastError());
    t->pending |= 2; t->last_actor_B = B;
    return EV2G_OK;
}

int ev2g_tqc_critic_grad(ev2g_handle *h, ev2g_tqc *t, const float *obs, const float *actions, const float *reward, const float *next_obs,
                         const uint8_t *done, int B, float *losses) {
    return tqc_critic_stage(h, t, "ev2g_tqc_critic_grad", obs, actions, reward, next_obs, done, B, losses);
}
int ev2g_tqc_actor_grad(ev2g_handle *h, ev2g_tqc *t, const float *obs, int B, float *losses) { return tqc_actor_stage(h, t, "ev2g_tqc_actor_grad", obs, B, losses); }
int ev2g_tqc_apply(ev2g_handle *h, ev2g_tqc *t) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_apply")) return rc;
    return sac_apply_stage(h, t, "ev2g_tqc_apply");
}
int ev2g_tqc_update(ev2g_handle *h, ev2g_tqc *t, const float *obs, const float *actions, const float *reward, const float *next_obs,
                    const uint8_t *done, int B, float *losses) {
    const char *who = "ev2g_tqc_update";
    if (int rc = tqc_critic_stage(h, t, who, obs, actions, reward, next_obs, done, B, losses)) return rc;
    if (int rc = sac_apply_stage(h, t, who)) return rc;
    if (int rc = tqc_actor_stage(h, t, who, obs, B, losses)) return rc;
    return sac_apply_stage(h, t, who);
}
int ev2g_tqc_act(ev2g_handle *h, ev2g_tqc *t, const float *obs32, int n_rows, int deterministic, float *actions, float *mu, float *log_std, float *log_pi) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_act")) return rc;
    return core_act(h, t, "ev2g_tqc_act", obs32, n_rows, deterministic, actions, mu, log_std, log_pi);
}
int ev2g_tqc_collect(ev2g_handle *h, ev2g_tqc *t, int k_steps, int deterministic, const ev2g_transitions *tr) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_collect")) return rc;
    return core_collect(h, t, "ev2g_tqc_collect", k_steps, deterministic, tr);
}
int ev2g_tqc_get_grads(ev2g_handle *h, ev2g_tqc *t, float *const *out, float *g_log_ent_coef) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_get_grads")) return rc;
    return core_get_grads(h, t, "ev2g_tqc_get_grads", out, g_log_ent_coef);
}
int ev2g_tqc_get_weights(ev2g_handle *h, ev2g_tqc *t, int target, float *const *out) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_get_weights")) return rc;
    return core_get_weights(h, t, "ev2g_tqc_get_weights", target, out);
}
int ev2g_tqc_get_z(ev2g_handle *h, ev2g_tqc *t, float *z, float *log_pi_next, int B) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_get_z")) return rc;
    return sac_read_rows(h, "ev2g_tqc_get_z", z, t->work + t->tq.w_z, log_pi_next, t->work + t->tq.w_lp2, B, t->last_B, t->tq.K);
}
int ev2g_tqc_get_log_pi(ev2g_handle *h, ev2g_tqc *t, float *log_pi, int B) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_get_log_pi")) return rc;
    return sac_read_rows(h, "ev2g_tqc_get_log_pi", log_pi, t->work + t->tq.w_lp, nullptr, nullptr, B, t->last_actor_B);
}
int ev2g_tqc_get_ent_coef(ev2g_handle *h, ev2g_tqc *t, float *out3) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_get_ent_coef")) return rc;
    return core_get_ent_coef(h, t, "ev2g_tqc_get_ent_coef", out3);
}
int ev2g_tqc_set_rate(ev2g_handle *h, ev2g_tqc *t, double lr) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_set_rate")) return rc;
    return core_set_rate(h, t, "ev2g_tqc_set_rate", lr);
}
int ev2g_tqc_seed(ev2g_handle *h, ev2g_tqc *t, uint64_t seed, uint64_t first_draw) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_seed")) return rc;
    t->seed = seed; t->next_draw = first_draw;
    return EV2G_OK;
}
int ev2g_tqc_act_seed(ev2g_handle *h, ev2g_tqc *t, uint64_t seed, uint64_t first_launch) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_act_seed")) return rc;
    t->act_seed = seed; t->act_n = first_launch;
    return EV2G_OK;
}
int ev2g_tqc_counters(ev2g_handle *h, ev2g_tqc *t, int64_t *updates, int64_t *target_updates, uint64_t *next_draw, uint64_t *act_launches) {
    if (int rc = tqc_check(h, t, "ev2g_tqc_counters")) return rc;
    return core_counters(t, updates, target_updates, next_draw, act_launches);
}

// the quantile arguments of ev2g_tqc_truncate and of the host twins: plan_tqc's refusal on the smallest network, or B's
static std::string tqc_atoms_refusal(const char *who, int B, int nc, int nq, int drop) {
    const TqcPlan p = plan_tqc(1, 1, 1, 1, nc, nq, drop);
    if (p.err) return std::string(who) + ": " + p.refusal;
    return td3_batch_refusal(who, B);
}
int ev2g_tqc_truncate(ev2g_handle *h, const float *tq, const float *log_pi_next, const float *reward, const uint8_t *done, int B, int n_critics,
                      int n_quantiles, int top_quantiles_to_drop, double gamma, const float *log_ent_coef, float *z_out) {
    const char *who = "ev2g_tqc_truncate";
    if (!h) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    if (!tq || !log_pi_next || !reward || !done || !log_ent_coef || !z_out) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    const std::string refusal = tqc_atoms_refusal(who, B, n_critics, n_quantiles, top_quantiles_to_drop);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    (void)hipSetDevice(h->device);
    tqc_launch_target(h, tq, log_pi_next, reward, done, B, n_critics, n_quantiles, n_critics * (n_quantiles - top_quantiles_to_drop), gamma, log_ent_coef, z_out);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_host_tqc_target(const float *tq, const float *log_pi_next, const float *reward, const uint8_t *done, int B, int n_critics, int n_quantiles,
                         int top_quantiles_to_drop, double gamma, float log_ent_coef, float *z) {
    if (!tq || !log_pi_next || !reward || !done || !z) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_tqc_target: null argument");
    const std::string refusal = tqc_atoms_refusal("ev2g_host_tqc_target", B, n_critics, n_quantiles, top_quantiles_to_drop);
    if (!refusal.empty()) return fail(nullptr, EV2G_ERR_ARG, refusal);
    tqc_host_target(tq, log_pi_next, reward, done, B, n_critics, n_quantiles, top_quantiles_to_drop, gamma, log_ent_coef, z);
    return EV2G_OK;
}
int ev2g_host_tqc_critic_head(const float *z, const float *q, int B, int n_critics, int n_quantiles, int top_quantiles_to_drop, float *dq,
                              float *critic_loss) {
    if (!z || !q || !dq || !critic_loss) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_tqc_critic_head: null argument");
    const std::string refusal = tqc_atoms_refusal("ev2g_host_tqc_critic_head", B, n_critics, n_quantiles, top_quantiles_to_drop);
    if (!refusal.empty()) return fail(nullptr, EV2G_ERR_ARG, refusal);
    *critic_loss = tqc_host_critic_head(z, q, B, n_critics, n_quantiles, n_critics * (n_quantiles - top_quantiles_to_drop), dq);
    return EV2G_OK;
}

int ev2g_check_faults(ev2g_handle *h, int32_t *first_bad_env) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_check_faults: no scenarios loaded");
    (void)hipSetDevice(h->device);
    std::vector<int> f(h->E);
    HIPCHK(h, hipMemcpyAsync(f.data(), h->st.env_fault, sizeof(int) * h->E, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int e = 0; e < h->E; e++)
        if (f[e]) {
            if (first_bad_env) *first_bad_env = e;
            return fail(h, EV2G_ERR_OVERCURRENT, "charger over-current: sum of amps is higher than max charge current (ev_charger.py:203-205)");
        }
    return EV2G_OK;
}

static int launch_stats(ev2g_handle *h, double *stats, bool reset, double *obs, long long off, float *obs32 = nullptr) {
    (void)hipSetDevice(h->device);
    // the step launch that closed the episode computed the statistics (and nothing has changed the state since): copy them
    const bool copy = h->last.inl_stats && h->current_step == h->T;
    h->last_stats_route = copy ? 1 : 0;
    h->stats_reason = copy ? "" : h->last.inl_reason;
    if (copy && !reset) {
        HIPCHK(h, hipMemcpyAsync(stats, h->d_stats_inl, sizeof(double) * (size_t)h->E * EV2G_N_STATS, hipMemcpyDeviceToDevice, h->stream));
        return EV2G_OK;
    }

    const bool pair = stats_pair(h);
    const dim3 grid(pair ? (h->E + 1) / 2 : h->E);
    if (copy) {   // reset-only: the rows are copied (the in-launch shapes are those with one env per wavefront)
        hipLaunchKernelGGL((ev2g_copy_stats_reset_kernel<1>), dim3(h->E), dim3(64), 0, h->stream, h->scn, h->st, (const double *)h->d_stats_inl, stats, (int)off, obs,
                           obs32 ? obs32 : (float *)h->extras.obs_f32);
        HIPCHK(h, hipGetLastError());
        return EV2G_OK;
    }
#define EV2G_STATS_LAUNCH(EPWS, RESET)                                                                                                    \
    hipLaunchKernelGGL((ev2g_stats_kernel<EPWS, RESET>), grid, dim3(64), (size_t)EV2G_STATS_LK * 64 * sizeof(double), h->stream, h->scn, h->st, (int)h->scn_off, (const double *)h->d_ss_afap, \
                       h->current_step, stats, (int)off, obs, RESET ? (obs32 ? obs32 : (float *)h->extras.obs_f32) : (float *)nullptr)
    if (pair) { if (reset) EV2G_STATS_LAUNCH(2, true); else EV2G_STATS_LAUNCH(2, false); }
    else { if (reset) EV2G_STATS_LAUNCH(1, true); else EV2G_STATS_LAUNCH(1, false); }
#undef EV2G_STATS_LAUNCH
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_get_stats(ev2g_handle *h, double *stats) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_get_stats: no scenarios loaded");
    if (!stats) return fail(h, EV2G_ERR_ARG, "ev2g_get_stats: null output");
    return launch_stats(h, stats, false, nullptr, 0);
}

static int stats_reset_impl(ev2g_handle *h, double *stats, double *obs, float *obs32, int64_t scenario_offset) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_get_stats_reset: no scenarios loaded");
    if (!stats) return fail(h, EV2G_ERR_ARG, "ev2g_get_stats_reset: null output");
    long long off = scenario_offset % (long long)h->scn.M;
    if (off < 0) off += h->scn.M;
    const int rc = launch_stats(h, stats, true, obs, off, obs32);
    if (rc) return rc;
    if (h->st.cs_power_hist) {
        HIPCHK(h, hipMemsetAsync(h->st.cs_power_hist, 0, sizeof(double) * (size_t)h->scn.T * h->scn.E * h->scn.C, h->stream));
        HIPCHK(h, hipMemsetAsync(h->st.cs_cur_hist, 0, sizeof(double) * (size_t)h->scn.T * h->scn.E * h->scn.C, h->stream));
    }
    h->scn_off = off;
    h->current_step = 0;
    state_changed(h, "the episode was reset");
    return EV2G_OK;
}
int ev2g_get_stats_reset(ev2g_handle *h, double *stats, double *obs, int64_t scenario_offset) { return stats_reset_impl(h, stats, obs, nullptr, scenario_offset); }
int ev2g_get_stats_reset_f32(ev2g_handle *h, double *stats, float *obs32, int64_t scenario_offset) { return stats_reset_impl(h, stats, nullptr, obs32, scenario_offset); }

// ---- the ARS learner and its population actor (ev2g_ars.h) ----
static int ars_check(ev2g_handle *h, ev2g_ars *a, const char *who) { return owned_check(h, &ev2g_handle::arss, a, "ARS learner", who, false); }

struct ArsActEntry {
    const void *fn;
    void (*launch)(const LaunchDims &, const ArsDev &, const float *images, const float *x, int R, float *act);
};
extern "C++" template <int KIND>
static void launch_ars_act(const LaunchDims &d, const ArsDev &dev, const float *images, const float *x, int R, float *act) {
    hipLaunchKernelGGL(ev2g_ars_act_kernel<KIND>, d.grid, dim3(EV2G_AC_BLOCK), d.lds, d.stream, dev, images, x, R, act);
}
static const ArsActEntry &ars_act_kernel(int kind) {
    static const ArsActEntry tab[2] = {{(const void *)ev2g_ars_act_kernel<EV2G_ARS_MLP>, &launch_ars_act<EV2G_ARS_MLP>},
                                       {(const void *)ev2g_ars_act_kernel<EV2G_ARS_LINEAR>, &launch_ars_act<EV2G_ARS_LINEAR>}};
    return tab[kind == EV2G_ARS_LINEAR ? 1 : 0];
}
static unsigned ars_blocks(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 1 << 16); }

// one launch of ev2g_ars_act_kernel over n_rows rows: C = 2 n_delta candidates of n_rows / C rows over the candidate images, or the centre image
static int ars_launch(ev2g_handle *h, ev2g_ars *a, const float *x, int n_rows, bool population, float *actions) {
    const int C = population ? 2 * a->plan.n_delta : 1, R = n_rows / C;
    const LaunchDims dims{dim3((unsigned)(C * ars_tiles_per_candidate(R))), a->plan.lds, h->stream};
    ars_act_kernel(a->plan.kind).launch(dims, a->dev, population ? a->cand : a->centre, x, R, actions);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

int ev2g_ars_default_config(ev2g_ars_config *cfg) {
    if (!cfg) return fail(nullptr, EV2G_ERR_ARG, "ev2g_ars_default_config: cfg is null");
    ars_default_config(cfg);
    return EV2G_OK;
}

int ev2g_ars_query(const ev2g_ars_config *cfg, int kind, int d_in, int h1, int h2, int d_out, ev2g_ars_info *out) {
    if (!cfg || !out) return fail(nullptr, EV2G_ERR_ARG, "ev2g_ars_query: null argument");
    const std::string refusal = ars_config_refusal("ev2g_ars_query", *cfg);
    if (!refusal.empty()) return fail(nullptr, EV2G_ERR_ARG, refusal);
    const ArsPlan p = plan_ars(kind, d_in, h1, h2, d_out, cfg->n_delta, cfg->n_top);
    if (p.err) return fail(nullptr, p.err, p.refusal);
    *out = ev2g_ars_info{EV2G_AC_MAX_IN, EV2G_AC_MAX_HIDDEN, EV2G_AC_MAX_OUT, EV2G_ARS_MAX_DELTA, p.lay.n_params, (int64_t)p.dev.stride,
                         (int64_t)p.image_bytes, (int64_t)p.delta_bytes, (int64_t)p.total_bytes, (int64_t)p.lds};
    return EV2G_OK;
}

static int ars_launch_repack(ev2g_handle *h, ev2g_ars *a) {
    hipLaunchKernelGGL(ev2g_ars_repack_kernel, dim3(ars_blocks(a->plan.lay.n_params)), dim3(256), 0, h->stream, a->plan.lay, (const float *)a->theta, a->centre);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}

static int ars_device_stage(ev2g_handle *h, ev2g_ars *a, const float *theta) {
    const ArsPlan &p = a->plan;
    const size_t n = (size_t)p.lay.n_params, nd = (size_t)p.n_delta, stride = (size_t)p.dev.stride;
    if (int rc = dalloc(h, a->allocs, n, &a->theta)) return rc;
    if (int rc = dalloc(h, a->allocs, stride, &a->centre)) return rc;          // (zeros: the padding nothing writes afterwards)
    if (int rc = dalloc(h, a->allocs, 2 * nd * stride, &a->cand)) return rc;
    if (int rc = dalloc(h, a->allocs, nd * n, &a->delta)) return rc;
    if (int rc = dalloc(h, a->allocs, 2 * nd, &a->ret)) return rc;
    if (int rc = dalloc(h, a->allocs, nd, &a->rank)) return rc;
    if (int rc = dalloc(h, a->allocs, nd, &a->order)) return rc;
    if (int rc = dalloc(h, a->allocs, 1, &a->report)) return rc;
    if (theta) HIPCHK(h, hipMemcpyAsync(a->theta, theta, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (int rc = ars_launch_repack(h, a)) return rc;
    const unsigned bit = 1u << (p.kind == EV2G_ARS_LINEAR ? 1 : 0);
    if (p.lds > 48 * 1024 && !(h->ars_attr_mask & bit)) {   // (function attributes are per device: once per handle, for the largest network)
        const hipError_t e = hipFuncSetAttribute(ars_act_kernel(p.kind).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ev2g_sac_lds_max());
        if (e != hipSuccess) return fail(h, EV2G_ERR_HIP, std::string("ev2g_ars_create: hipFuncSetAttribute: ") + hipGetErrorString(e));
        h->ars_attr_mask |= bit;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));   // theta is the caller's
    return EV2G_OK;
}

int ev2g_ars_create(ev2g_handle *h, const ev2g_ars_config *cfg, int kind, int d_in, int h1, int h2, int d_out, float lo, const float *theta, uint64_t seed,
                    ev2g_ars **out) {
    const char *who = "ev2g_ars_create";
    if (!h || !out) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    *out = nullptr;
    if (!cfg) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    const std::string refusal = ars_config_refusal(who, *cfg);
    if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
    const ArsPlan plan = plan_ars(kind, d_in, h1, h2, d_out, cfg->n_delta, cfg->n_top);
    if (plan.err) return fail(h, plan.err, plan.refusal);
    if (lo != -1.0f && lo != 0.0f) return fail(h, EV2G_ERR_ARG, std::string(who) + ": lo must be -1 or 0");
    if (theta)
        for (int i = 0; i < plan.lay.n_params; i++)
            if (!std::isfinite(theta[i])) return fail(h, EV2G_ERR_ARG, std::string(who) + ": theta[" + std::to_string(i) + "] is not finite");
    (void)hipSetDevice(h->device);
    ev2g_ars *a = new ev2g_ars();
    a->cfg = *cfg; a->plan = plan; a->dev = plan.dev; a->dev.lo = lo; a->seed = seed;
    return owned_created(h, &ev2g_handle::arss, a, ars_device_stage(h, a, theta), out);
}

void ev2g_ars_destroy(ev2g_handle *h, ev2g_ars *a) { owned_destroy(h, &ev2g_handle::arss, a); }

int ev2g_ars_perturb(ev2g_handle *h, ev2g_ars *a) {
    if (int rc = ars_check(h, a, "ev2g_ars_perturb")) return rc;
    const ArsPlan &p = a->plan;
    hipLaunchKernelGGL(ev2g_ars_perturb_kernel, dim3(ars_blocks((long long)p.n_delta * p.lay.n_params)), dim3(256), 0, h->stream, p.lay, (const float *)a->theta,
                       p.n_delta, (float)a->cfg.delta_std, (uint64_t)a->seed, (uint64_t)a->iter, (long long)p.dev.stride, a->delta, a->cand);
    HIPCHK(h, hipGetLastError());
    if (a->env_return) HIPCHK(h, hipMemsetAsync(a->env_return, 0, (size_t)a->rows_E * sizeof(double), h->stream));
    a->iter += 1; a->steps = 0; a->roll_E = 0; a->have_dirs = true; a->returns_set = false;
    return EV2G_OK;
}

int ev2g_ars_act(ev2g_handle *h, ev2g_ars *a, const float *obs32, int n_rows, int population, float *actions) {
    const char *who = "ev2g_ars_act";
    if (int rc = ars_check(h, a, who)) return rc;
    if (!obs32 || !actions || n_rows <= 0) return fail(h, EV2G_ERR_ARG, std::string(who) + ": obs32 or actions is null, or n_rows is not positive");
    if (population) {
        const std::string refusal = ars_rows_refusal(who, "n_rows", n_rows, a->plan.n_delta);
        if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
        if (!a->have_dirs) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no candidates yet (ev2g_ars_perturb first)");
    }
    return ars_launch(h, a, obs32, n_rows, population != 0, actions);
}

// the object's rows for the loaded shape: the observation and action rows, the envs' returns and the reward rows of one episode
static int ars_rows(ev2g_handle *h, ev2g_ars *a, const char *who) {
    if (!h->loaded) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no scenarios loaded");
    if (a->obs32 && a->rows_E == h->E && a->rows_D == h->D && a->rows_P == h->P && a->rows_T == h->T) return EV2G_OK;
    if (a->roll_E) return fail(h, EV2G_ERR_STATE, std::string(who) + ": the loaded shape changed inside an iteration (ev2g_ars_perturb starts the next one)");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    free_pool(a->swap_allocs);
    a->obs32 = a->act32 = nullptr; a->env_return = a->reward = nullptr; a->done = a->mask = nullptr;
    a->rows_E = h->E; a->rows_D = h->D; a->rows_P = h->P; a->rows_T = h->T;
    if (int rc = dalloc(h, a->swap_allocs, (size_t)h->E * h->D, &a->obs32)) return rc;
    if (int rc = dalloc(h, a->swap_allocs, (size_t)h->E * h->P, &a->act32)) return rc;
    if (int rc = dalloc(h, a->swap_allocs, (size_t)h->E, &a->env_return)) return rc;
    if (int rc = dalloc(h, a->swap_allocs, (size_t)h->E, &a->done)) return rc;
    if (int rc = dalloc(h, a->swap_allocs, (size_t)h->E * h->P, &a->mask)) return rc;
    return dalloc(h, a->swap_allocs, (size_t)h->E * h->T, &a->reward);
}

float *ev2g_ars_obs_f32(ev2g_handle *h, ev2g_ars *a) {
    if (ars_check(h, a, "ev2g_ars_obs_f32") || ars_rows(h, a, "ev2g_ars_obs_f32")) return nullptr;
    return a->obs32;
}
float *ev2g_ars_actions_f32(ev2g_handle *h, ev2g_ars *a) {
    if (ars_check(h, a, "ev2g_ars_actions_f32") || ars_rows(h, a, "ev2g_ars_actions_f32")) return nullptr;
    return a->act32;
}

int ev2g_ars_rollout(ev2g_handle *h, ev2g_ars *a, int k_steps, int population, double *reward, int64_t r_stride) {
    const char *who = "ev2g_ars_rollout";
    if (int rc = ars_check(h, a, who)) return rc;
    if (!h->loaded) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no scenarios loaded");
    if (k_steps < 0 || (reward && r_stride < h->E)) return fail(h, EV2G_ERR_ARG, std::string(who) + ": negative step count, or a reward stride below the env count");
    if (a->dev.d_in != h->D) return fail(h, EV2G_ERR_ARG, std::string(who) + ": d_in " + std::to_string(a->dev.d_in) + " != the observation width " + std::to_string(h->D));
    if (a->dev.d_out != h->P) return fail(h, EV2G_ERR_ARG, std::string(who) + ": d_out " + std::to_string(a->dev.d_out) + " != the ports " + std::to_string(h->P));
    if (population) {
        const std::string refusal = ars_rows_refusal(who, "the env count", h->E, a->plan.n_delta);
        if (!refusal.empty()) return fail(h, EV2G_ERR_ARG, refusal);
        if (!a->have_dirs) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no candidates yet (ev2g_ars_perturb first)");
    }
    const ev2g_step_extras &x = h->extras;
    const bool direct = collect_direct(h);   // the two routes of ev2g_ac_collect
    if (!direct && !(x.obs_f32 && x.actions_f32 && x.obs_f32_step_stride == 0))
        return fail(h, EV2G_ERR_ARG, std::string(who) + ": this configuration steps through the registered float32 hand-over buffers: register them with "
                                                        "ev2g_set_step_extras (observation step stride 0) first");
    if (int rc = ars_rows(h, a, who)) return rc;
    StepChain c{who};
    c.ars = a; c.ars_population = population != 0; c.ars_direct = direct;
    c.reward = reward ? Rows<double>{reward, (long long)r_stride} : Rows<double>{a->reward, h->E};
    c.done = {a->done}; c.mask = {a->mask};   // (stride 0: the per-launch float32 rows need the full instantiation, which writes every output)
    c.count_steps = false;   // (as ev2g_ac_collect: the registered buffers do not advance)
    if (int rc = run_chain(h, c, k_steps)) return rc;
    if (k_steps > 0 && population) {   // (a centre rollout is no part of the iteration: the envs' returns, the step count and roll_E stay as they are)
        hipLaunchKernelGGL(ev2g_ars_returns_kernel, dim3((unsigned)((h->E + 255) / 256)), dim3(256), 0, h->stream, a->env_return, (const double *)c.reward.p, k_steps,
                           c.reward.stride, h->E);
        HIPCHK(h, hipGetLastError());
        a->steps += k_steps; a->roll_E = h->E;
    }
    return EV2G_OK;
}

int ev2g_ars_update(ev2g_handle *h, ev2g_ars *a) {
    const char *who = "ev2g_ars_update";
    if (int rc = ars_check(h, a, who)) return rc;
    const ArsPlan &p = a->plan;
    if (!a->have_dirs) return fail(h, EV2G_ERR_STATE, std::string(who) + ": no directions yet (ev2g_ars_perturb first)");
    if (!a->returns_set && !a->roll_E)
        return fail(h, EV2G_ERR_STATE, std::string(who) + ": no returns yet (ev2g_ars_rollout in population mode, or ev2g_ars_set_returns, first)");
    if (!a->returns_set) {
        const int C = 2 * p.n_delta;
        hipLaunchKernelGGL(ev2g_ars_candidates_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, h->stream, (const double *)a->env_return, a->roll_E / C, C,
                           a->cfg.alive_bonus_offset, a->steps, a->ret);
    }
    hipLaunchKernelGGL(ev2g_ars_rank_kernel, dim3(1), dim3(256), 0, h->stream, (const double *)a->ret, p.n_delta, p.n_top, a->cfg.learning_rate,
                       (long long)a->iter - 1, a->rank, a->order, a->report);
    hipLaunchKernelGGL(ev2g_ars_step_kernel, dim3(ars_blocks(p.lay.n_params)), dim3(256), 0, h->stream, p.lay, a->theta, (const float *)a->delta,
                       (const double *)a->ret, (const int32_t *)a->order, (const ev2g_ars_report *)a->report, p.n_delta, p.n_top, a->centre);
    HIPCHK(h, hipGetLastError());
    a->updates += 1; a->returns_set = false; a->roll_E = 0;
    return EV2G_OK;
}

int ev2g_ars_get_report(ev2g_handle *h, ev2g_ars *a, ev2g_ars_report *report, double *returns, int32_t *ranks) {
    if (int rc = ars_check(h, a, "ev2g_ars_get_report")) return rc;
    if (report) HIPCHK(h, hipMemcpyAsync(report, a->report, sizeof *report, hipMemcpyDeviceToHost, h->stream));
    if (returns) HIPCHK(h, hipMemcpyAsync(returns, a->ret, (size_t)2 * a->plan.n_delta * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (ranks) HIPCHK(h, hipMemcpyAsync(ranks, a->rank, (size_t)a->plan.n_delta * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}

static int ars_read(ev2g_handle *h, const char *who, void *dst, const void *src, size_t bytes) {
    if (!dst) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
int ev2g_ars_get_weights(ev2g_handle *h, ev2g_ars *a, float *theta) {
    if (int rc = ars_check(h, a, "ev2g_ars_get_weights")) return rc;
    return ars_read(h, "ev2g_ars_get_weights", theta, a->theta, (size_t)a->plan.lay.n_params * sizeof(float));
}
int ev2g_ars_set_weights(ev2g_handle *h, ev2g_ars *a, const float *theta) {
    const char *who = "ev2g_ars_set_weights";
    if (int rc = ars_check(h, a, who)) return rc;
    if (!theta) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    for (int i = 0; i < a->plan.lay.n_params; i++)
        if (!std::isfinite(theta[i])) return fail(h, EV2G_ERR_ARG, std::string(who) + ": theta[" + std::to_string(i) + "] is not finite");
    HIPCHK(h, hipMemcpyAsync(a->theta, theta, (size_t)a->plan.lay.n_params * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (int rc = ars_launch_repack(h, a)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));   // theta is the caller's
    return EV2G_OK;
}
int ev2g_ars_get_candidate(ev2g_handle *h, ev2g_ars *a, int c, float *theta) {
    const char *who = "ev2g_ars_get_candidate";
    if (int rc = ars_check(h, a, who)) return rc;
    if (c < 0 || c >= 2 * a->plan.n_delta) return fail(h, EV2G_ERR_ARG, std::string(who) + ": candidate " + std::to_string(c) + " is outside 0 .. " + std::to_string(2 * a->plan.n_delta - 1));
    std::vector<float> image((size_t)a->plan.dev.stride);
    if (int rc = ars_read(h, who, theta ? image.data() : nullptr, a->cand + (size_t)c * (size_t)a->plan.dev.stride, image.size() * sizeof(float))) return rc;
    ars_unpack(a->plan.lay, image.data(), theta);
    return EV2G_OK;
}
int ev2g_ars_get_deltas(ev2g_handle *h, ev2g_ars *a, float *delta) {
    if (int rc = ars_check(h, a, "ev2g_ars_get_deltas")) return rc;
    return ars_read(h, "ev2g_ars_get_deltas", delta, a->delta, (size_t)a->plan.n_delta * a->plan.lay.n_params * sizeof(float));
}
int ev2g_ars_get_env_returns(ev2g_handle *h, ev2g_ars *a, double *env_return, int n_envs) {
    const char *who = "ev2g_ars_get_env_returns";
    if (int rc = ars_check(h, a, who)) return rc;
    if (!a->env_return || n_envs != a->rows_E) return fail(h, EV2G_ERR_ARG, std::string(who) + ": n_envs is not the env count of the object's rollouts");
    return ars_read(h, who, env_return, a->env_return, (size_t)n_envs * sizeof(double));
}
int ev2g_ars_set_returns(ev2g_handle *h, ev2g_ars *a, const double *returns) {
    const char *who = "ev2g_ars_set_returns";
    if (int rc = ars_check(h, a, who)) return rc;
    if (!returns) return fail(h, EV2G_ERR_ARG, std::string(who) + ": null argument");
    HIPCHK(h, hipMemcpyAsync(a->ret, returns, (size_t)2 * a->plan.n_delta * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // returns is the caller's
    a->returns_set = true;
    return EV2G_OK;
}
int ev2g_ars_set_rates(ev2g_handle *h, ev2g_ars *a, double learning_rate, double delta_std) {
    if (int rc = ars_check(h, a, "ev2g_ars_set_rates")) return rc;
    if (int rc = fields_check(h, "ev2g_ars_set_rates", ars_rate_fields(learning_rate, delta_std))) return rc;
    a->cfg.learning_rate = learning_rate; a->cfg.delta_std = delta_std;
    return EV2G_OK;
}
int ev2g_ars_seed(ev2g_handle *h, ev2g_ars *a, uint64_t seed, uint64_t first_iteration) {
    if (int rc = ars_check(h, a, "ev2g_ars_seed")) return rc;
    a->seed = seed; a->iter = first_iteration;
    return EV2G_OK;
}
int ev2g_ars_counters(ev2g_handle *h, ev2g_ars *a, uint64_t *next_iteration, int64_t *updates, int64_t *steps) {
    if (int rc = ars_check(h, a, "ev2g_ars_counters")) return rc;
    if (next_iteration) *next_iteration = a->iter;
    if (updates) *updates = a->updates;
    if (steps) *steps = a->steps;
    return EV2G_OK;
}

int ev2g_host_ars_perturb(const float *theta, int n_delta, int n_params, double delta_std, uint64_t seed, uint64_t iteration, float *delta, float *cand) {
    if (!theta || !delta) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_ars_perturb: null argument");
    if (n_delta < 1 || n_params < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_ars_perturb: n_delta and n_params must be positive");
    ars_host_perturb(theta, n_delta, n_params, delta_std, seed, iteration, delta, cand, [](uint64_t s, uint64_t j) { return ev2g_ac_normal(s, j); });
    return EV2G_OK;
}
int ev2g_host_ars_returns(double *env_return, const double *reward, int k, int64_t r_stride, int n_envs, int n_candidates, double alive_bonus_offset,
                          int64_t steps, double *returns) {
    if (!env_return) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_ars_returns: null argument");
    if (k < 0 || n_envs < 1 || (reward && r_stride < n_envs) || (returns && (n_candidates < 1 || n_envs % n_candidates != 0)))
        return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_ars_returns: k < 0, a stride below n_envs, or n_envs is no multiple of n_candidates");
    ars_host_returns(env_return, reward, k, (long long)r_stride, n_envs, n_candidates, alive_bonus_offset, (long long)steps, returns);
    return EV2G_OK;
}
int ev2g_host_ars_update(float *theta, const float *delta, const double *returns, int n_delta, int n_top, int n_params, double learning_rate, int32_t *ranks,
                         ev2g_ars_report *report) {
    if (!theta || !delta || !returns || !ranks || !report) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_ars_update: null argument");
    if (n_delta < 1 || n_top < 1 || n_top > n_delta || n_params < 1) return fail(nullptr, EV2G_ERR_ARG, "ev2g_host_ars_update: 1 <= n_top <= n_delta and n_params >= 1 are needed");
    report->iteration = 0; report->reserved = 0;
    ars_host_update(theta, delta, returns, n_delta, n_top, n_params, learning_rate, ranks, report);
    return EV2G_OK;
}

// ---- multi-GPU statistics exchange (RCCL) --------------------------------------------------------------------------------
int ev2g_comm_get_unique_id(void *id) {
    RcclApi *api = rccl_api();
    if (!api->lib) return fail(nullptr, EV2G_ERR_STATE, "ev2g_comm_get_unique_id: " + api->err);
    if (!id) return fail(nullptr, EV2G_ERR_ARG, "ev2g_comm_get_unique_id: null output");
    static_assert(sizeof(ncclUniqueId) == EV2G_COMM_ID_BYTES, "EV2G_COMM_ID_BYTES must be sizeof(ncclUniqueId)");
    ncclUniqueId u;
    const ncclResult_t r = api->GetUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, EV2G_ERR_HIP, std::string("ncclGetUniqueId: ") + api->GetErrorString(r));
    std::memcpy(id, &u, sizeof u);
    return EV2G_OK;
}

int ev2g_comm_init(ev2g_handle *h, const void *id, int rank, int world_size) {
    if (!h) return fail(h, EV2G_ERR_ARG, "ev2g_comm_init: null handle");
    if (!id || world_size < 1 || rank < 0 || rank >= world_size) return fail(h, EV2G_ERR_ARG, "ev2g_comm_init: bad arguments");
    RcclApi *api = rccl_api();
    if (!api->lib) return fail(h, EV2G_ERR_STATE, "ev2g_comm_init: " + api->err);
    ev2g_comm_destroy(h);
    (void)hipSetDevice(h->device);
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    const ncclResult_t r = api->CommInitRank(&h->comm.comm, world_size, u, rank);
    if (r != ncclSuccess) { h->comm.comm = nullptr; return fail(h, EV2G_ERR_HIP, std::string("ncclCommInitRank: ") + api->GetErrorString(r)); }
    h->comm.rank = rank; h->comm.world = world_size;
    return EV2G_OK;
}

void ev2g_comm_destroy(ev2g_handle *h) {
    if (!h || !h->comm.comm) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    rccl_api()->CommDestroy(h->comm.comm);
    if (h->comm.d_send) (void)hipFree(h->comm.d_send);
    h->comm = CommState{};
}

int ev2g_comm_world_size(const ev2g_handle *h) { return (h && h->comm.comm) ? h->comm.world : 0; }
long long ev2g_comm_gathers(const ev2g_handle *h) { return h ? h->comm.gathers : 0; }

int ev2g_gather_stats(ev2g_handle *h, double *stats_all) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_gather_stats: no scenarios loaded");
    if (!h->comm.comm) return fail(h, EV2G_ERR_STATE, "ev2g_gather_stats: no communicator (call ev2g_comm_init on every rank first)");
    if (!stats_all) return fail(h, EV2G_ERR_ARG, "ev2g_gather_stats: null output");
    (void)hipSetDevice(h->device);
    if (h->comm.send_envs != h->E) {
        if (h->comm.d_send) { (void)hipStreamSynchronize(h->stream); (void)hipFree(h->comm.d_send); h->comm.d_send = nullptr; }
        HIPCHK(h, hipMalloc((void **)&h->comm.d_send, sizeof(double) * (size_t)h->E * EV2G_N_STATS));
        h->comm.send_envs = h->E;
    }
    RcclApi *api = rccl_api();
    if (h->comm.checked_envs != h->E) {
        // ncclAllGather needs the same count on every rank: verify it once per communicator / loaded batch, with a collective whose
        // own count cannot differ (one int per rank), instead of gathering mismatched blocks into the wrong rows.  Every rank gets here
        // on its first gather after ev2g_comm_init (ranks that reload a batch of another size must do so together).
        int *d_n = nullptr;
        HIPCHK(h, hipMalloc((void **)&d_n, sizeof(int) * (size_t)(h->comm.world + 1)));
        HIPCHK(h, hipMemcpyAsync(d_n, &h->E, sizeof(int), hipMemcpyHostToDevice, h->stream));
        const ncclResult_t rn = api->AllGather(d_n, d_n + 1, 1, ncclInt32, h->comm.comm, h->stream);
        std::vector<int> n(h->comm.world + 1, 0);
        hipError_t he = hipMemcpyAsync(n.data(), d_n, sizeof(int) * n.size(), hipMemcpyDeviceToHost, h->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(h->stream);
        (void)hipFree(d_n);
        if (rn != ncclSuccess) return fail(h, EV2G_ERR_HIP, std::string("ncclAllGather (env counts): ") + api->GetErrorString(rn));
        HIPCHK(h, he);
        for (int r = 0; r < h->comm.world; r++)
            if (n[r + 1] != h->E)
                return fail(h, EV2G_ERR_STATE, "ev2g_gather_stats: rank " + std::to_string(r) + " steps " + std::to_string(n[r + 1]) + " envs, this rank " +
                                                   std::to_string(h->E) + " (the gather needs equal shards; pad the batch or use torch's uneven gather)");
        h->comm.checked_envs = h->E;
    }
    const int rc = ev2g_get_stats(h, h->comm.d_send);
    if (rc) return rc;
    const ncclResult_t r = api->AllGather(h->comm.d_send, stats_all, (size_t)h->E * EV2G_N_STATS, ncclDouble, h->comm.comm, h->stream);
    if (r != ncclSuccess) return fail(h, EV2G_ERR_HIP, std::string("ncclAllGather: ") + api->GetErrorString(r));
    h->comm.gathers++;
    return EV2G_OK;
}

int ev2g_peek(ev2g_handle *h, int env, ev2g_env_view *v) {
    if (!h || !h->loaded) return fail(h, EV2G_ERR_STATE, "ev2g_peek: no scenarios loaded");
    if (!v || env < 0 || env >= h->E) return fail(h, EV2G_ERR_ARG, "ev2g_peek: bad arguments");
    if (h->refilled) return fail(h, EV2G_ERR_STATE, "ev2g_peek: the scenario pool was refilled on the device (ev2g_pool_refill): the host holds no copy of its scenarios");
    (void)hipSetDevice(h->device);
    const int P = h->P, C = h->C, R = h->R, T = h->T, E = h->E;
    const DevState &st = h->st;
    std::vector<double> cap(P), tot(P), prev(P);
    std::vector<int2> win(P), sc(P);
    const size_t off = (size_t)env * P;
#define D2H(dst, src, n, type) HIPCHK(h, hipMemcpyAsync((dst), (src), sizeof(type) * (size_t)(n), hipMemcpyDeviceToHost, h->stream))
    // One env's pieces come down into ONE page-locked staging block (kept with the handle): copies into pageable vectors are staged by the runtime one
    // after the other (~15 us each; the facade peeks after every step: round 6, 0.19 -> 0.05 ms per call), these are queued together and waited for once.
    const bool log_cs = st.cs_profits != nullptr;
    const size_t n_lines = (size_t)P * sizeof(PortLine) / 8, n_hist = (size_t)T * (2 + R);
    const size_t need = 8 * (n_lines + 2 * (size_t)P + (size_t)R + (log_cs ? 5 * (size_t)C : 0) + n_hist);
    if (h->peek_stage_bytes < need) {
        if (h->peek_stage) { (void)hipHostFree(h->peek_stage); h->peek_stage = nullptr; h->peek_stage_bytes = 0; }
        HIPCHK(h, hipHostMalloc(&h->peek_stage, need, hipHostMallocDefault));
        h->peek_stage_bytes = need;
    }
    double *stg = (double *)h->peek_stage;
    const PortLine *lines = (const PortLine *)stg;
    double *pe = stg + n_lines, *pc = pe + P, *trp = pc + P, *csv = trp + R, *hist_rows = csv + (log_cs ? 5 * (size_t)C : 0);
    D2H((void *)lines, st.line + off, P, PortLine);
    D2H(pe, st.port_energy + off, P, double);
    D2H(pc, st.port_current + off, P, double);
    D2H(trp, st.tr_power_now + (size_t)env * R, R, double);
    if (log_cs) {
        D2H(csv + 0 * C, st.cs_power_now + (size_t)env * C, C, double);
        D2H(csv + 1 * C, st.cs_cur_now + (size_t)env * C, C, double);
        D2H(csv + 2 * C, st.cs_profits + (size_t)env * C, C, double);
        D2H(csv + 3 * C, st.cs_e_ch + (size_t)env * C, C, double);
        D2H(csv + 4 * C, st.cs_e_dis + (size_t)env * C, C, double);
    }
    std::vector<double> usage(T), pot(T), over((size_t)T * R);
    D2H(hist_rows, st.hist + (size_t)env * T * (2 + R), n_hist, double);   // this env's rows of the history array [E, T, 2 + R]: contiguous
#undef D2H
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // rows the running episode has not written yet read as zeros (the reference's arrays are zero-initialised at reset); the slab itself may still
    // hold the previous episode's values there -- after an in-kernel reset of a fused run, and after ev2g_get_stats_reset, which re-arms an env
    // without clearing its history rows (the statistics kernel ignores them the same way).  usage / overload of step t exist once step t has run,
    // the charge-power potential of step t once step t - 1 has.
    const int cur = h->current_step;
    for (int t = 0; t < T; t++) {
        usage[t] = (t < cur) ? hist_rows[(size_t)t * (2 + R)] : 0.0;
        pot[t] = (t <= cur) ? hist_rows[(size_t)t * (2 + R) + 1] : 0.0;
        for (int r = 0; r < R; r++) over[(size_t)t * R + r] = (t < cur) ? hist_rows[(size_t)t * (2 + R) + 2 + r] : 0.0;
    }
    for (int q = 0; q < P; q++) {
        const PortLine &l = lines[q];
        cap[q] = l.cap; tot[q] = l.tot; prev[q] = l.prev; win[q] = make_int2(l.ta, l.td); sc[q] = make_int2(l.ss, ev2g_line_cycles(l.cyc_lut));
    }
    const int t = h->current_step;
    v->current_step = t;
    v->n_ports = P; v->n_chargers = C; v->n_transformers = R; v->n_steps = T;
    const long long scn = ((long long)env + h->scn_off) % h->M;   // the scenario this env is running
    const long long s0 = h->env_sess_start[scn], s1 = h->env_sess_start[scn + 1];
    std::vector<int> dev_to_local;  // device idx -> env-local host idx
    if (v->port_session) {
        // inverse map restricted to this env
        int dmin = 0x7fffffff;
        for (long long s = s0; s < s1; s++) dmin = std::min(dmin, h->host_to_dev[s]);
        dev_to_local.assign((size_t)(s1 - s0), -1);
        for (long long s = s0; s < s1; s++) dev_to_local[h->host_to_dev[s] - dmin] = (int)(s - s0);
        for (int q = 0; q < P; q++) {
            const bool occ = win[q].x <= t && t <= win[q].y && sc[q].x >= 0;
            v->port_session[h->slot_port[q]] = occ ? dev_to_local[sc[q].x - dmin] : -1;
        }
    }
    const double nan = std::nan("");
    for (int q = 0; q < P; q++) {
        const int p = h->slot_port[q];
        // after step t-1 the port holds an EV iff its window covers the current step counter
        const bool occ = win[q].x <= t && t <= win[q].y;
        if (v->port_capacity) v->port_capacity[p] = occ ? cap[q] : nan;
        if (v->port_energy) v->port_energy[p] = occ ? pe[q] : nan;
        if (v->port_current) v->port_current[p] = occ ? pc[q] : nan;
        if (v->port_total_energy) v->port_total_energy[p] = occ ? tot[q] : nan;
        if (v->port_prev_power) v->port_prev_power[p] = occ ? prev[q] : nan;
        if (v->port_required_energy) v->port_required_energy[p] = nan;  // filled by the Python facade (B - cap0 - tot_e)
        if (v->port_cycles) v->port_cycles[p] = occ ? sc[q].y : -1;
    }
    for (int c = 0; c < C; c++) {
        if (v->cs_power) v->cs_power[c] = log_cs ? csv[0 * C + c] : nan;
        if (v->cs_amps) v->cs_amps[c] = log_cs ? csv[1 * C + c] : nan;
        if (v->cs_profits) v->cs_profits[c] = log_cs ? csv[2 * C + c] : nan;
        if (v->cs_energy_charged) v->cs_energy_charged[c] = log_cs ? csv[3 * C + c] : nan;
        if (v->cs_energy_discharged) v->cs_energy_discharged[c] = log_cs ? csv[4 * C + c] : nan;
    }
    // entries the running episode has not written yet read as zeros (after an in-kernel reset of a fused run the slab still holds the
    // previous episode's values there); charge_power_potential is written one step ahead (utils.py:760-791)
    for (int k = t; k < T; k++) { usage[k] = 0.0; for (int r = 0; r < R; r++) over[(size_t)k * R + r] = 0.0; }
    for (int k = t + 1; k < T; k++) pot[k] = 0.0;
    if (v->tr_power) std::copy(trp, trp + R, v->tr_power);
    if (v->tr_overload)
        for (int r = 0; r < R; r++)
            for (int k = 0; k < T; k++) v->tr_overload[(size_t)r * T + k] = over[(size_t)k * R + r];
    if (v->power_usage) std::copy(usage.begin(), usage.end(), v->power_usage);
    if (v->power_potential) std::copy(pot.begin(), pot.end(), v->power_potential);
    std::vector<double> fcap;
    if (v->session_final_cap && s1 > s0) {
        int dmin = 0x7fffffff;
        for (long long s = s0; s < s1; s++) dmin = std::min(dmin, h->host_to_dev[s]);
        fcap.resize((size_t)(s1 - s0));
        HIPCHK(h, hipMemcpy(fcap.data(), st.sess_final_cap + dmin, sizeof(double) * (size_t)(s1 - s0), hipMemcpyDeviceToHost));
        for (long long s = s0; s < s1; s++) v->session_final_cap[s - s0] = fcap[h->host_to_dev[s] - dmin];
    }
    for (long long s = s0; s < s1; s++) {
        if (v->session_port) v->session_port[s - s0] = h->sess_port[s];
        if (v->session_afap) v->session_afap[s - s0] = h->sess_afap[s];
    }
    return EV2G_OK;
}

#ifdef EV2G_PHASE_TIMING
int ev2g_debug_phase_ticks(ev2g_handle *h, unsigned long long *out18) {
    std::vector<unsigned long long> v((size_t)h->scn.n_groups * 18);
    HIPCHK(h, hipMemcpy(v.data(), h->st.dbg, v.size() * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < 18; i++) { out18[i] = 0; for (int b = 0; b < h->scn.n_groups; b++) out18[i] += v[(size_t)b * 18 + i]; }
    HIPCHK(h, hipMemset(h->st.dbg, 0, v.size() * 8));
    return 0;
}
#endif

void *ev2g_malloc(ev2g_handle *h, size_t bytes) {
    if (!h) return nullptr;
    (void)hipSetDevice(h->device);
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(bytes, 1)) != hipSuccess) {
        h->err = "ev2g_malloc: hipMalloc failed";
        return nullptr;
    }
    h->user_allocs.push_back(p);
    return p;
}
void ev2g_free(ev2g_handle *h, void *p) {
    if (!h || !p) return;
    auto it = std::find(h->user_allocs.begin(), h->user_allocs.end(), p);
    if (it != h->user_allocs.end()) h->user_allocs.erase(it);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(p);
}
void *ev2g_host_malloc(ev2g_handle *h, size_t bytes) {
    if (!h) return nullptr;
    (void)hipSetDevice(h->device);
    void *p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) {
        h->err = "ev2g_host_malloc: hipHostMalloc failed";
        return nullptr;
    }
    h->user_host_allocs.push_back(p);
    return p;
}
void ev2g_host_free(ev2g_handle *h, void *p) {
    if (!h || !p) return;
    auto it = std::find(h->user_host_allocs.begin(), h->user_host_allocs.end(), p);
    if (it == h->user_host_allocs.end()) return;   // (not ours, or freed already)
    h->user_host_allocs.erase(it);
    (void)hipStreamSynchronize(h->stream);
    (void)hipHostFree(p);
}
int ev2g_memcpy_h2d(ev2g_handle *h, void *dst, const void *src, size_t bytes) {
    if (!h) return EV2G_ERR_ARG;
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
int ev2g_memcpy_d2h(ev2g_handle *h, void *dst, const void *src, size_t bytes) {
    if (!h) return EV2G_ERR_ARG;
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
int ev2g_synchronize(ev2g_handle *h) {
    if (!h) return EV2G_ERR_ARG;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EV2G_OK;
}
int ev2g_fill_uniform(ev2g_handle *h, double *dst, int64_t n, uint64_t seed, double lo, double hi) {
    if (!h || !dst || n < 0) return fail(h, EV2G_ERR_ARG, "ev2g_fill_uniform: bad arguments");
    (void)hipSetDevice(h->device);
    const int nb = (int)std::min<int64_t>((n + 255) / 256, 2048);
    if (n) hipLaunchKernelGGL(ev2g_fill_uniform_kernel, dim3(std::max(nb, 1)), dim3(256), 0, h->stream, dst, (long long)n, seed, lo, hi);
    HIPCHK(h, hipGetLastError());
    return EV2G_OK;
}
void ev2g_host_uniform(double *dst, int64_t n, uint64_t seed, double lo, double hi) {
    for (int64_t i = 0; i < n; i++) dst[i] = lo + (hi - lo) * ev2g_u01(seed, (uint64_t)i);
}

// ---- scenario generator (host only) ----
int ev2g_gen_default_config(int kind, ev2g_gen_config *cfg) { return ev2g_gen_default_config_impl(kind, cfg); }
int ev2g_pool_refill(ev2g_handle *h, const ev2g_gen_config *cfg, uint64_t seed, int64_t first_index, int32_t first_slot, int32_t n) {
    if (h) state_changed(h, "scenarios were refilled since the last step launch");
    try { return ev2g_pool_refill_impl(h, cfg, seed, first_index, first_slot, n); }
    catch (const std::exception &e) { return fail(h, EV2G_ERR_ARG, std::string("ev2g_pool_refill: ") + e.what()); }
}
long long ev2g_pool_refill_overflows(ev2g_handle *h) { return ev2g_pool_refill_overflows_impl(h); }
int ev2g_pool_session_capacity(const ev2g_handle *h) { return h ? h->sess_cap : 0; }
int ev2g_generate(const ev2g_gen_config *cfg, int32_t n_scenarios, uint64_t seed, int32_t n_threads, ev2g_gen_result **out) {
    return ev2g_generate_impl(cfg, n_scenarios, seed, n_threads, out);
}
const ev2g_scenario_batch *ev2g_gen_batch(const ev2g_gen_result *r) { return r ? &r->b : nullptr; }
void ev2g_gen_free(ev2g_gen_result *r) { delete r; }
int ev2g_gen_table(int which, int kind, double *out, int n_max) { return ev2g_gen_table_impl(which, kind, out, n_max); }

}  // extern "C"
