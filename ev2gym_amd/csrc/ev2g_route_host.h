// ev2g_route_host.h -- the host-only half of a step launch: which kernel instantiation it gets and what it computes on the side.
//
// ev2g_load_scenarios fixes a RouteShape (the kernel family and everything of the loaded batch a route depends on); every launch passes a
// RouteCall (which buffers are there, their strides, what is registered in the extras, t0 / k / auto_reset -- presence and sizes, no
// pointers).  route_step(shape, call) is the whole decision: the instantiation, the number ev2g_last_launch_specialisation reports, whether
// the launch fast-forwards EV-free stretches and computes the episode statistics in its tail, and the two "why not" strings.  route_fused
// is the same for the one-launch rollout segment, collect_direct the collectors' rule.  ev2g_host.hip is the device stage: it fills the
// two structs, calls the function, stores the result and makes one launch from a table.  Nothing here needs HIP, a handle or a kernel
// header, so a plain C++17 program can enumerate the decision (tests/host/route_check.cpp).
//
// The kernels restate two of these rules on their side (ev2g_step_wave.h: FFW, INL) from what they are passed: V2P::ff_count / stats_inl
// set by the loader, k, t0 and T.  A change here that widens either needs the kernel's half widened too.
#pragma once
#include <algorithm>

#include "../../include/ev2g.h"
#include "ev2g_timing_host.h"

// the kernel a launch runs on
enum RouteFamily {
    ROUTE_GENERIC = 0,   // ev2g_step_kernel: more than 1024 ports, or chargers with different port counts
    ROUTE_V2,            // ev2g_step_v2<block, SPEC>
    ROUTE_BIG,           // a load: ev2g_step_v2<1024> whose specialised launches run on ev2g_step_big; a launch: ev2g_step_big
    ROUTE_WAVE           // ev2g_step_wave: the common shape
};

// What ev2g_load_scenarios fixed (load_route, load_route_big, load_params and load_decide_inl_stats fill it in).
struct RouteShape {
    int family = ROUTE_GENERIC;
    int block = 0;              // ev2g_step_v2's block for this port count (256 / 512 / 1024; the fast path's window table follows it too), 0: none
    int P = 0, T = 0, D = 0, npc = 0;
    int state_kind = 0, reward_kind = 0, flags = 0;   // ev2g_config's
    bool pow2_dt = false;       // 60 / timescale is a power of two (15, 30, 60 minutes): compiled into ev2g_step_v2<.., 1>
    int epw = 1;                // ev2g_step_wave: envs per wavefront (WaveArgs::epw; the lane stride between them is P)
    // EV2G_NO_FULL (or more than 4094 efficiency tables: the full kernels keep table id + 1 in 12 bits of a port's LDS word) / EV2G_NO_WIDE /
    // EV2G_NO_STRIDED / EV2G_NO_INLAUNCH_STATS at load time: A/B runs, routing and parity tests
    bool no_full = false, no_wide = false, no_strided = false, no_inl_stats = false;
    bool ff_count = false;      // V2P::ff_count is set: the fast path with one env per wavefront, no EV2G_NO_FAST_FORWARD
    bool stats_inl = false;     // V2P::stats_inl is set: the shape has the in-launch statistics phase ...
    const char *inl_shape_reason = "";   // ... why not
    bool balance = false;       // the handle builds CU-balance maps (ev2g_balance_host.h): ff_count, T <= 256, not EV2G_FLAG_REFILLABLE, no EV2G_NO_CU_BALANCE ...
    const char *balance_shape_reason = "";   // ... why not
    bool wave() const { return family == ROUTE_WAVE; }
    bool big() const { return family == ROUTE_BIG; }
};

// What one launch passes: StepIO's buffers and strides, the registered extras, the steps.
struct RouteCall {
    bool actions = false, act32 = false, obs = false, obs32 = false, reward = false, done = false, mask = false;   // StepIO's pointers are non-null
    long long a_stride = 0, o_stride = 0, r_stride = 0, d_stride = 0, m_stride = 0;
    bool x_cost = false, x_obs_f32 = false, x_actions_f32 = false;   // ev2g_set_step_extras
    long long x_cost_stride = 0, x_obs_f32_stride = 0;
    int t0 = 0, k = 0, auto_reset = 0;
};

struct StepRoute {
    int family = ROUTE_GENERIC;
    int sk = 0, rk = 0, fullk = 0;   // ROUTE_WAVE: ev2g_step_wave<sk, rk, io32, fullk> (rk: the reward's slot, 3 = the run-time rewards' shared one)
    bool io32 = false;
    int block = 0;                   // ROUTE_V2: ev2g_step_v2<block, spec>
    bool spec = false;
    int specialisation = -1;         // ev2g_last_launch_specialisation
    bool ff = false;                 // the kernel fast-forwards and counts (ev2g_last_launch_fast_forwarded)
    bool balance = false;            // the launch gets a CU-balance map for the window it steps (ev2g_last_launch_balance) ...
    const char *balance_reason = ""; // ... why it keeps the kernel's own map
    bool inl_stats = false;          // the kernel computes get_statistics of every env in its tail
    bool stamps = false;             // the instantiation has the two launch-stamp sites (timing_wave_stamped, ev2g_timing_host.h: the kernel's STAMPED is the same function)
    const char *general_reason = ""; // ev2g_last_launch_general_reason
    const char *inl_reason = "";     // why the in-launch statistics are not available (ev2g_last_stats_reason reports it)
    const char *refusal = nullptr;   // the launch is refused (EV2G_ERR_ARG) with this message: nothing above `ff` is decided then
};

// rewards beyond the three compiled-in ones share slot 3
inline int route_reward_slot(int reward_kind) { return std::min(reward_kind, 3); }

// The instantiations of ev2g_step_wave that step launches use, as a table index and back: the general one (fullk 0) for every pair and
// both action formats; full (1) and full + wide (2) for the compiled-in rewards; wide with strided outputs (3) for those, float64 only.
constexpr int ROUTE_WAVE_ENTRIES = 3 * 4 * 2 * 4;
constexpr int route_wave_index(int sk, int rk, bool io32, int fullk) { return ((sk * 4 + rk) * 2 + (io32 ? 1 : 0)) * 4 + fullk; }
constexpr bool route_wave_exists(int sk, int rk, bool io32, int fullk) {
    return sk >= 0 && sk < 3 && rk >= 0 && rk < 4 && fullk >= 0 && fullk < 4 && (fullk == 0 || (rk != 3 && (fullk != 3 || !io32)));
}

inline StepRoute route_step(const RouteShape &s, const RouteCall &c) {
    StepRoute r;
    r.inl_reason = r.balance_reason = "the step kernel is not ev2g_step_wave";
    const bool cs_hist = (s.flags & EV2G_FLAG_LOG_CS_HISTORY) != 0, log_soc = (s.flags & EV2G_FLAG_LOG_SOC) != 0;
    const bool strided = c.o_stride != 0 || c.r_stride != 0 || c.d_stride != 0 || c.m_stride != 0;
    if (s.wave()) {
        r.family = ROUTE_WAVE;
        // the fast path advances its output pointers by 32-bit byte strides
        const long long lim = 1ll << 32;
        if (c.a_stride * 8 >= lim || c.o_stride * 8 >= lim || c.r_stride * 8 >= lim || c.d_stride >= lim || c.m_stride >= lim ||
            c.x_cost_stride * 8 >= lim || c.x_obs_f32_stride * 4 >= lim || c.a_stride < 0 || c.o_stride < 0 || c.r_stride < 0 ||
            c.d_stride < 0 || c.m_stride < 0 || c.x_cost_stride < 0 || c.x_obs_f32_stride < 0) {
            r.refusal = "ev2g_step_n: a step stride is negative or reaches 4 GiB (unsupported by the fast-path kernel)";
            return r;
        }
        const int rk = route_reward_slot(s.reward_kind);
        // every float64 output present, no extras, no charger histories: the specialisation without their checks (not for the run-time rewards)
        // ... in two flavours: float64 actions in / float64 observations out (a loop that consumes them, the benchmark), or the policy
        // network's hand-over, float32 actions in / float32 observations out and no float64 observation (ev2g_rollout)
        const bool f64io = c.actions && c.obs && !c.x_obs_f32, f32io = !c.actions && c.act32 && !c.obs && c.obs32;
        const bool full0 = (f64io || f32io) && c.reward && c.done && c.mask && !c.x_cost && !cs_hist && !c.auto_reset && c.t0 + c.k <= s.T &&
                           rk != 3 && !s.no_full;
        // ... and: SoC log on, one observation-head column pair per lane at most (PublicPST has no head table), three lanes for the history store
        const bool wide0 = full0 && log_soc && s.P >= 3 && !s.no_wide &&
                           s.P >= (s.state_kind == EV2G_STATE_PUBLIC_PST ? 3 : (s.state_kind == EV2G_STATE_V2G_PROFIT_MAX_LOADS ? 30 : 10));
        // outputs with step strides ([K, E, *] blocks): the wide float64 instantiation with running output pointers (3); elsewhere stride 0 only
        const bool str3 = strided && wide0 && f64io && !s.no_strided;
        const bool full = full0 && (!strided || str3), wide = wide0 && full;
        r.sk = s.state_kind; r.rk = rk;
        r.fullk = full ? (str3 ? 3 : (wide ? 2 : 1)) : 0;
        r.io32 = full ? f32io : !c.actions;
        r.specialisation = r.fullk;
        r.stamps = timing_wave_stamped(r.fullk);
        // (ev2g_step_wave.h's FFW is the kernel's half: a stride-0 float64 full instantiation of a head-table state, V2P::ff_count set -- one env per
        // wavefront --, k > 1)
        r.ff = full && !str3 && f64io && c.k > 1 && s.ff_count && s.state_kind != EV2G_STATE_PUBLIC_PST;
        // CU balance: the launches that fast-forward, from step 0 (a group's weight is its live steps of the whole episode)
        if (!r.ff) r.balance_reason = "the launch does not fast-forward (ev2g_last_launch_fast_forwarded: a persistent stride-0 float64 launch of more than one step, one env per wavefront)";
        else if (c.t0 != 0) r.balance_reason = "the launch does not start at step 0";
        else if (!s.balance) r.balance_reason = s.balance_shape_reason;
        else r.balance_reason = "";
        r.balance = r.balance_reason[0] == 0;
        // why not the full instantiation: the FIRST thing the caller passed (or configured) that rules it out
        if (!full) {
            if (s.no_full) r.general_reason = "EV2G_NO_FULL is set (or the batch has more than 4094 efficiency tables)";
            else if (rk == 3) r.general_reason = "the reward function is one of the eight selected at run time (only the shipped configs' three are compiled in)";
            else if (cs_hist) r.general_reason = "EV2G_FLAG_LOG_CS_HISTORY (charger histories)";
            else if (c.x_cost) r.general_reason = "a cost buffer is registered (ev2g_set_step_extras)";
            else if (c.auto_reset) r.general_reason = "auto_reset";
            else if (!(c.reward && c.done && c.mask)) r.general_reason = "a reward / done / mask output is NULL";
            else if (!(f64io || f32io)) r.general_reason = "the observation / action buffers are neither the float64 pair nor the float32 hand-over pair (e.g. obs NULL, or a float32 observation copy next to the float64 one)";
            else if (strided) r.general_reason = "an output step stride is not 0 (strided outputs keep the specialisation only with float64 observations, EV2G_FLAG_LOG_SOC and an env wide enough for the wide instantiation)";
            else r.general_reason = "the launch would run past the episode end";
        }
        // a launch of the float64 wide instantiation (2) that ends the episode computes its statistics in its tail (ev2g_step_wave.h's INL is the
        // kernel's half: V2P::stats_inl set, k > 1, the launch ends at T)
        if (s.no_inl_stats) r.inl_reason = "EV2G_NO_INLAUNCH_STATS is set";
        else if (c.t0 + c.k != s.T) r.inl_reason = "the last step launch did not end the episode";
        else if (c.k < 2) r.inl_reason = "the episode ended in a single-step launch (per-step launches keep the statistics kernel)";
        else if (!(wide && !str3 && f64io)) r.inl_reason = "the last step launch was not the float64 wide instantiation with step stride 0 (ev2g_last_launch_specialisation 2)";
        else if (!s.stats_inl) r.inl_reason = s.inl_shape_reason;
        else r.inl_reason = "";
        r.inl_stats = r.inl_reason[0] == 0;
        return r;
    }
    // the general kernel's instantiation for the default plugin pair launched with everything present (ev2g_step_v2.h, SPEC); big envs run
    // it on ev2g_step_big (512 threads, two ports per home lane, two workgroups per CU)
    const bool v2 = s.family == ROUTE_V2 || s.family == ROUTE_BIG;
    r.spec = v2 && s.state_kind == EV2G_STATE_V2G_PROFIT_MAX_LOADS && s.reward_kind == 0 && s.npc == 1 && c.actions && c.obs && c.reward &&
             c.done && c.mask && !c.x_cost && !c.x_obs_f32 && !cs_hist && log_soc && !strided && !c.auto_reset && c.t0 + c.k <= s.T && s.pow2_dt &&
             !s.no_full;
    r.family = !v2 ? ROUTE_GENERIC : (r.spec && s.big()) ? ROUTE_BIG : ROUTE_V2;
    r.block = v2 ? s.block : 0;
    r.specialisation = v2 ? (r.spec ? (s.big() ? 5 : 1) : 0) : -1;
    return r;
}

// The collectors' route (ev2g_collect's unfused loop, ev2g_ac_collect): true where a one-step launch can take float32 action and observation
// rows of its own (StepIO::act32 / obs32) and gets the full instantiation for them -- the fast path with nothing registered, no charger
// histories, a compiled-in reward; elsewhere the step works on the registered hand-over pair and the rows are copied around it.  A rule of
// its own, stricter than "full" (nothing registered at all): tests/host/route_check.cpp holds it against route_step.
inline bool collect_direct(const RouteShape &s, bool x_cost, bool x_obs_f32, bool x_actions_f32) {
    return s.wave() && !x_cost && !x_obs_f32 && !x_actions_f32 && !(s.flags & EV2G_FLAG_LOG_CS_HISTORY) && route_reward_slot(s.reward_kind) != 3 && !s.no_full;
}

// ---- one launch per rollout segment: ev2g_step_wave<.., 2, 1024, true, AE, NWF> evaluates the policy between the steps, inside the launch ----
// the streaming actor's fragment packing (ev2g_mlp: 0s when the network runs on another kernel); nw: bf16 terms per weight
struct FusedPacking { int ks1 = 0, nt1 = 0, nt2 = 0, nt3 = 0, nw = 0; };
struct FusedRoute {
    bool eligible = false;
    int ae = 1, nwf = 1;   // envs per wavefront, bf16 terms per weight (2: the float32 policy)
    int index = -1;        // the instantiation's table entry, and its bit in the handle's function-attribute mask
};
// The fused instantiations as a table index and back: [0, 16) state kind * 4 + reward for the bf16 policy with one env per wavefront,
// [16, 20) PublicPST with two, [20, 32) 20 + state kind * 4 + reward for the float32 policy; the reward slots 3 stay empty.
constexpr int ROUTE_FUSED_ENTRIES = 32;
constexpr int route_fused_index(int sk, int rk, int ae, int nwf) { return nwf == 2 ? 20 + sk * 4 + rk : (ae == 2 ? 16 + rk : sk * 4 + rk); }
struct FusedKey { int sk, rk, ae, nwf; bool exists; };
constexpr FusedKey route_fused_key(int i) {
    return i < 16 ? FusedKey{i / 4, i % 4, 1, 1, i / 4 < 3 && i % 4 < 3}
         : i < 20 ? FusedKey{EV2G_STATE_PUBLIC_PST, i - 16, 2, 1, i - 16 < 3}
                  : FusedKey{(i - 20) / 4, (i - 20) % 4, 1, 2, (i - 20) / 4 < 3 && (i - 20) % 4 < 3};
}

// Eligible: the fast path (3..64 ports: the shipped YAMLs' 25 chargers, BASELINE configs[1] / configs[4]'s 50; every env gets a wavefront of
// its own in this instantiation, whatever its width -- PublicPST envs of at most 32 ports go two to a wavefront under the bf16 policy), one of
// the three compiled-in rewards, EV2G_FLAG_LOG_SOC, no extras beyond the float32 hand-over, and the policy in the streaming kernel's packing
// for the state: PublicPST's 3 + 3 P <= 63 inputs and P <= 20 outputs in 64 -> 400 -> 300 -> 32, the head-table states (an even row width)
// in 192 -> 400 -> 300 -> 64; bf16, or float32 as two bf16 terms per weight.  Anything else, EV2G_NO_FUSED=1 and (the float32 policy)
// EV2G_NO_FUSED_F32=1 keep the two launches per step; the two switches are read per call by the caller.
inline FusedRoute route_fused(const RouteShape &s, bool x_cost, const FusedPacking &m, bool no_fused, bool no_fused_f32) {
    FusedRoute r;
    const bool pst = s.state_kind == EV2G_STATE_PUBLIC_PST;
    const int rk = route_reward_slot(s.reward_kind);
    r.eligible = s.wave() && s.P >= 3 && s.P <= 64 && rk != 3 && (s.flags & EV2G_FLAG_LOG_SOC) && !(s.flags & EV2G_FLAG_LOG_CS_HISTORY) && !x_cost &&
                 !s.no_full && !s.no_wide && (pst || (s.D & 1) == 0) && m.ks1 == (pst ? 2 : 6) && m.nt1 == 25 && m.nt2 == 19 && m.nt3 == (pst ? 2 : 4) &&
                 (m.nw == 1 || (m.nw == 2 && !no_fused_f32)) && !no_fused;
    r.ae = (pst && s.P <= 32 && m.nw == 1) ? 2 : 1;
    r.nwf = m.nw;
    r.index = r.eligible ? route_fused_index(s.state_kind, rk, r.ae, r.nwf) : -1;
    return r;
}
