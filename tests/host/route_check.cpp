// route_check.cpp -- enumerates a step launch's route (ev2gym_amd/csrc/ev2g_route_host.h) and checks every output of route_step,
// collect_direct and route_fused against predicates written here from the contract's wording (include/ev2g.h: ev2g_last_launch_specialisation,
// ev2g_last_launch_general_reason, ev2g_last_stats_route, ev2g_last_launch_fast_forwarded), each a flat condition on the
// inputs.  Exits non-zero at the first failure.
//
//   c++ -std=c++17 -O1 -ffp-contract=off tests/host/route_check.cpp -o route_check && ./route_check
//
// (tests/test_route_cpu.py does exactly that; the same source builds with -fsanitize=address,undefined.)
//
// The inputs: every boolean of RouteShape and RouteCall (the two config flags a route reads among them), the four families, the three state
// kinds, reward kinds 0..3 and 7, two ports-per-charger counts, each of the seven strides zero / non-zero / negative / 4 GiB, the three
// auto_reset values, P in {2, 3, 9, 10, 29, 30, 64} and (t0, k) in {(0, 1), (0, T), (T - 1, 1), (T - 2, 2), (T - 1, 2)}.  Their full cross
// product has some 1e14 points, so it is covered by two sweeps, each exhaustive in one half of the dimensions while the other half is drawn
// per point from a counter-based hash (every value of it, paired with everything, many times over):
//   sweep 1: all 19 booleans x family x state kind, exhaustive (6.3 M points, twice with different draws);
//   sweep 2: family x state kind x reward x P x auto_reset x (t0, k) x the four output strides, and the same x the three input strides, exhaustive.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../ev2gym_amd/csrc/ev2g_route_host.h"

static const char *g_case = "";
static RouteShape g_shape;
static RouteCall g_call;
static void dump() {
    const RouteShape &s = g_shape;
    const RouteCall &c = g_call;
    std::fprintf(stderr, "  shape: family %d block %d P %d T %d D %d npc %d state %d reward %d flags %d pow2_dt %d epw %d no_full %d no_wide %d no_strided %d "
                         "no_inl_stats %d ff_count %d stats_inl %d\n", s.family, s.block, s.P, s.T, s.D, s.npc, s.state_kind, s.reward_kind, s.flags, s.pow2_dt,
                 s.epw, s.no_full, s.no_wide, s.no_strided, s.no_inl_stats, s.ff_count, s.stats_inl);
    std::fprintf(stderr, "  call: actions %d act32 %d obs %d obs32 %d reward %d done %d mask %d strides %lld %lld %lld %lld %lld extras %d %d %d strides %lld %lld "
                         "t0 %d k %d auto_reset %d\n", c.actions, c.act32, c.obs, c.obs32, c.reward, c.done, c.mask, c.a_stride, c.o_stride, c.r_stride,
                 c.d_stride, c.m_stride, c.x_cost, c.x_obs_f32, c.x_actions_f32, c.x_cost_stride, c.x_obs_f32_stride, c.t0, c.k, c.auto_reset);
}
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "FAIL [%s] line %d: %s\n", g_case, __LINE__, #cond);            \
            dump();                                                                              \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

static bool same(const char *a, const char *b) { return a && b && std::strcmp(a, b) == 0; }

// ---- the messages, as the GPU suite and the Python engine's warning read them ----
static const char *const kRefusal = "ev2g_step_n: a step stride is negative or reaches 4 GiB (unsupported by the fast-path kernel)";
static const char *const kNoFull = "EV2G_NO_FULL is set (or the batch has more than 4094 efficiency tables)";
static const char *const kRunTimeReward = "the reward function is one of the eight selected at run time (only the shipped configs' three are compiled in)";
static const char *const kCsHistory = "EV2G_FLAG_LOG_CS_HISTORY (charger histories)";
static const char *const kCost = "a cost buffer is registered (ev2g_set_step_extras)";
static const char *const kAutoReset = "auto_reset";
static const char *const kNullOutput = "a reward / done / mask output is NULL";
static const char *const kNoPair = "the observation / action buffers are neither the float64 pair nor the float32 hand-over pair (e.g. obs NULL, or a float32 observation copy next to the float64 one)";
static const char *const kStrided = "an output step stride is not 0 (strided outputs keep the specialisation only with float64 observations, EV2G_FLAG_LOG_SOC and an env wide enough for the wide instantiation)";
static const char *const kPastEnd = "the launch would run past the episode end";
static const char *const kNotWave = "the step kernel is not ev2g_step_wave";
static const char *const kNoInl = "EV2G_NO_INLAUNCH_STATS is set";
static const char *const kNotEnd = "the last step launch did not end the episode";
static const char *const kSingle = "the episode ended in a single-step launch (per-step launches keep the statistics kernel)";
static const char *const kNotTwo = "the last step launch was not the float64 wide instantiation with step stride 0 (ev2g_last_launch_specialisation 2)";
static const char *const kShapeReason = "several envs per wavefront (a shape reason of the test's own)";

// ---- the contract, restated: every quantity a flat condition on the inputs ----
struct Facts {
    bool wave, v2, big, refused;
    bool compiled_reward, cs_hist, log_soc, outputs, pair64, pair32, in_episode, out_strided, full_ok, wide_ok;
    int spec;
};
static const long long kGiB4 = 1ll << 32;
static bool bad_stride(long long elems, int bytes) { return elems < 0 || elems * bytes >= kGiB4; }

static Facts facts(const RouteShape &s, const RouteCall &c) {
    Facts f{};
    f.wave = s.family == ROUTE_WAVE; f.big = s.family == ROUTE_BIG; f.v2 = s.family == ROUTE_V2 || f.big;
    // the fast path addresses its rows by 32-bit byte offsets: float64 actions / observations / rewards / costs, float32 observation copies, byte done flags and masks
    f.refused = f.wave && (bad_stride(c.a_stride, 8) || bad_stride(c.o_stride, 8) || bad_stride(c.r_stride, 8) || bad_stride(c.d_stride, 1) ||
                           bad_stride(c.m_stride, 1) || bad_stride(c.x_cost_stride, 8) || bad_stride(c.x_obs_f32_stride, 4));
    f.compiled_reward = s.reward_kind <= EV2G_REWARD_PROFIT_MAXIMIZATION;
    f.cs_hist = (s.flags & EV2G_FLAG_LOG_CS_HISTORY) != 0; f.log_soc = (s.flags & EV2G_FLAG_LOG_SOC) != 0;
    f.outputs = c.reward && c.done && c.mask;
    f.pair64 = c.actions && c.obs && !c.x_obs_f32;          // float64 actions in and float64 observations out, no float32 copy next to them
    f.pair32 = !c.actions && !c.obs && c.act32 && c.obs32;  // the float32 hand-over and no float64 ones passed
    f.in_episode = c.t0 + c.k <= s.T;
    f.out_strided = c.o_stride != 0 || c.r_stride != 0 || c.d_stride != 0 || c.m_stride != 0;
    // 1 = "full": all outputs, one of the two pairs, no cost output, no charger histories, the launch ends within the episode, a compiled-in reward, no in-launch resets
    f.full_ok = f.outputs && (f.pair64 || f.pair32) && !c.x_cost && !f.cs_hist && f.in_episode && f.compiled_reward && c.auto_reset == 0 && !s.no_full;
    // 2 = full, plus the SoC log and an env wide enough for one observation-head column pair per lane (60 / 20 head columns; PublicPST: three lanes)
    const int wide_from = s.state_kind == EV2G_STATE_V2G_PROFIT_MAX_LOADS ? 30 : s.state_kind == EV2G_STATE_V2G_PROFIT_MAX ? 10 : 3;
    f.wide_ok = f.full_ok && f.log_soc && s.P >= wide_from && !s.no_wide;
    if (f.wave) {
        // 3 = 2 for float64 outputs with step strides, needs what 2 needs; EV2G_NO_STRIDED: strided outputs run 0; stride 0: 2, else 1, else 0
        if (f.out_strided) f.spec = (f.wide_ok && f.pair64 && !s.no_strided) ? 3 : 0;
        else f.spec = f.wide_ok ? 2 : f.full_ok ? 1 : 0;
    } else if (f.v2) {
        // the general kernel's one instantiation: the default plugin pair, single-port chargers, everything of the float64 list, the SoC log, 15 / 30 / 60-minute steps
        const bool one = s.state_kind == EV2G_STATE_V2G_PROFIT_MAX_LOADS && s.reward_kind == EV2G_REWARD_PROFITMAX_TRPENALTY_USERINCENTIVES && s.npc == 1 &&
                         f.outputs && c.actions && c.obs && !c.x_obs_f32 && !c.x_cost && !f.cs_hist && f.in_episode && c.auto_reset == 0 && !f.out_strided &&
                         f.log_soc && s.pow2_dt && !s.no_full;
        f.spec = one ? (f.big ? 5 : 1) : 0;
    } else f.spec = -1;
    return f;
}

// the first of these that holds is why a fast-path launch got the general instantiation
static const char *want_general_reason(const RouteShape &s, const RouteCall &c, const Facts &f) {
    const struct { bool holds; const char *why; } ladder[] = {
        {s.no_full, kNoFull}, {!f.compiled_reward, kRunTimeReward}, {f.cs_hist, kCsHistory}, {c.x_cost, kCost}, {c.auto_reset != 0, kAutoReset},
        {!f.outputs, kNullOutput}, {!(f.pair64 || f.pair32), kNoPair}, {f.out_strided, kStrided}, {true, kPastEnd}};
    for (const auto &l : ladder) if (l.holds) return l.why;
    return "";
}
// the first of these that holds is why the launch did not compute the statistics
static const char *want_inl_reason(const RouteShape &s, const RouteCall &c, const Facts &f) {
    const struct { bool holds; const char *why; } ladder[] = {
        {s.no_inl_stats, kNoInl}, {c.t0 + c.k != s.T, kNotEnd}, {c.k < 2, kSingle}, {!(f.spec == 2 && c.actions), kNotTwo}, {!s.stats_inl, s.inl_shape_reason}, {true, ""}};
    for (const auto &l : ladder) if (l.holds) return l.why;
    return "";
}

static long long g_points = 0;
static bool g_wave_seen[ROUTE_WAVE_ENTRIES];

static void check_point(const RouteShape &s, const RouteCall &c) {
    g_shape = s; g_call = c; g_points++;
    const StepRoute r = route_step(s, c);
    const Facts f = facts(s, c);
    // ---- predicate against function ----
    CHECK((r.refusal != nullptr) == f.refused);
    if (f.refused) {
        CHECK(same(r.refusal, kRefusal));
        CHECK(same(r.inl_reason, kNotWave) && !r.inl_stats && !r.ff);   // what the refused launch leaves for ev2g_last_stats_reason
        return;
    }
    CHECK(r.specialisation == f.spec);
    CHECK(r.family == (f.wave ? ROUTE_WAVE : !f.v2 ? ROUTE_GENERIC : f.spec == 5 ? ROUTE_BIG : ROUTE_V2));
    if (f.wave) {
        CHECK(r.sk == s.state_kind && r.rk == (f.compiled_reward ? s.reward_kind : 3) && r.fullk == f.spec && r.io32 == !c.actions);
        CHECK(route_wave_exists(r.sk, r.rk, r.io32, r.fullk));
        const int i = route_wave_index(r.sk, r.rk, r.io32, r.fullk);
        CHECK(i >= 0 && i < ROUTE_WAVE_ENTRIES);
        g_wave_seen[i] = true;
    }
    if (r.family == ROUTE_V2) CHECK(r.block == s.block && r.spec == (f.spec == 1));
    // a persistent launch of the stride-0 float64 specialisations 1 or 2, one env per wavefront (what sets ff_count), a head-table state
    const bool want_ff = f.wave && (f.spec == 1 || f.spec == 2) && c.actions && c.k > 1 && s.ff_count && s.state_kind != EV2G_STATE_PUBLIC_PST;
    CHECK(r.ff == want_ff);
    // a launch of specialisation 2 (float64) of more than one step ending at the last step, on a shape with the phase, unless switched off
    const bool want_inl = f.wave && f.spec == 2 && c.actions && c.k > 1 && c.t0 + c.k == s.T && s.stats_inl && !s.no_inl_stats;
    CHECK(r.inl_stats == want_inl);
    CHECK(same(r.general_reason, f.wave && f.spec == 0 ? want_general_reason(s, c, f) : ""));
    CHECK(same(r.inl_reason, f.wave ? want_inl_reason(s, c, f) : kNotWave));
    // ---- invariants ----
    const bool strided = f.out_strided, f64 = c.actions && c.obs;
    if (f.wave) CHECK((r.general_reason[0] == 0) == (r.specialisation != 0));
    CHECK((r.inl_reason[0] == 0) == r.inl_stats);
    if (r.inl_stats) CHECK(r.specialisation == 2 && f64 && !r.io32 && c.k > 1 && c.t0 + c.k == s.T);
    if (r.ff) CHECK((r.specialisation == 1 || r.specialisation == 2) && f64 && !r.io32 && !strided && c.k > 1 && s.state_kind != EV2G_STATE_PUBLIC_PST && s.ff_count);
    if (r.specialisation == 3) CHECK(f.wave && strided && f64 && !r.io32);
    if (r.specialisation == 5) CHECK(s.family == ROUTE_BIG && r.family == ROUTE_BIG);
    if (r.family == ROUTE_BIG) CHECK(r.specialisation == 5);
    if (r.specialisation == 2 || r.specialisation == 3) CHECK(f.log_soc);
}

// the collectors' one-step launch on the direct route: float32 rows of the call's own, nothing registered
static void check_direct(const RouteShape &s) {
    for (int xc = 0; xc < 2; xc++)
        for (int xo = 0; xo < 2; xo++)
            for (int xa = 0; xa < 2; xa++) {
                const bool direct = collect_direct(s, xc, xo, xa);
                // the fast path with nothing registered, no charger histories, a compiled-in reward
                CHECK(direct == (s.family == ROUTE_WAVE && !xc && !xo && !xa && !(s.flags & EV2G_FLAG_LOG_CS_HISTORY) &&
                                 s.reward_kind <= EV2G_REWARD_PROFIT_MAXIMIZATION && !s.no_full));
                if (!direct) continue;
                for (int t0 = 0; t0 < s.T; t0++) {
                    RouteCall c;
                    c.act32 = c.obs32 = c.reward = c.done = c.mask = true;
                    c.t0 = t0; c.k = 1;
                    g_shape = s; g_call = c;
                    const StepRoute r = route_step(s, c);
                    CHECK(!r.refusal && r.specialisation > 0 && r.io32 && r.family == ROUTE_WAVE);   // what the two run-time "internal:" checks guard
                }
            }
}

// ---- the fused launch ----
static FusedKey g_fused_seen[ROUTE_FUSED_ENTRIES];
static bool g_fused_hit[ROUTE_FUSED_ENTRIES];

static void check_fused(const RouteShape &s) {
    const FusedPacking packs[] = {{6, 25, 19, 4, 1}, {2, 25, 19, 2, 1}, {6, 25, 19, 4, 2}, {2, 25, 19, 2, 2}, {6, 25, 19, 4, 3}, {2, 25, 19, 2, 3},
                                  {0, 0, 0, 0, 0}, {6, 25, 19, 2, 1}, {2, 25, 19, 4, 1}, {6, 24, 19, 4, 1}, {6, 25, 18, 4, 1}};
    for (const FusedPacking &m : packs)
        for (int sw = 0; sw < 8; sw++) {
            const bool x_cost = sw & 1, no_fused = sw & 2, no_f32 = sw & 4;
            const FusedRoute r = route_fused(s, x_cost, m, no_fused, no_f32);
            const bool pst = s.state_kind == EV2G_STATE_PUBLIC_PST;
            // the fast path, 3..64 ports, a compiled-in reward, the SoC log, no extras beyond the hand-over, the wide full instantiation not switched off,
            // an even row width for the head-table states, the policy in the state's packing: bf16, or float32 as two terms
            const bool want = s.family == ROUTE_WAVE && s.P >= 3 && s.P <= 64 && s.reward_kind <= EV2G_REWARD_PROFIT_MAXIMIZATION && (s.flags & EV2G_FLAG_LOG_SOC) &&
                              !(s.flags & EV2G_FLAG_LOG_CS_HISTORY) && !x_cost && !s.no_full && !s.no_wide && (pst || s.D % 2 == 0) &&
                              m.nt1 == 25 && m.nt2 == 19 && (pst ? m.ks1 == 2 && m.nt3 == 2 : m.ks1 == 6 && m.nt3 == 4) &&
                              (m.nw == 1 || (m.nw == 2 && !no_f32)) && !no_fused;
            CHECK(r.eligible == want);
            if (!r.eligible) { CHECK(r.index == -1); continue; }
            CHECK(r.nwf == m.nw && r.ae == ((pst && s.P <= 32 && m.nw == 1) ? 2 : 1));   // PublicPST envs of at most 32 ports go two to a wavefront (bf16 policy)
            CHECK(r.index >= 0 && r.index < 32 && r.index < ROUTE_FUSED_ENTRIES);
            const FusedKey k = route_fused_key(r.index);
            CHECK(k.exists && k.sk == s.state_kind && k.rk == s.reward_kind && k.ae == r.ae && k.nwf == r.nwf);
            if (g_fused_hit[r.index]) {
                const FusedKey &o = g_fused_seen[r.index];
                CHECK(o.sk == k.sk && o.rk == k.rk && o.ae == r.ae && o.nwf == r.nwf);   // one entry, one instantiation
            }
            g_fused_hit[r.index] = true; g_fused_seen[r.index] = {s.state_kind, s.reward_kind, r.ae, r.nwf, true};
        }
}

// ---- the enumeration ----
static const int kT = 6;
static const int kFamilies[] = {ROUTE_GENERIC, ROUTE_V2, ROUTE_BIG, ROUTE_WAVE};
static const int kRewards[] = {0, 1, 2, 3, 7};
static const int kPorts[] = {2, 3, 9, 10, 29, 30, 64};
static const long long kStrides[] = {0, 320, -320, 1ll << 32};
static const int kT0K[][2] = {{0, 1}, {0, kT}, {kT - 1, 1}, {kT - 2, 2}, {kT - 1, 2}};

static uint64_t mix(uint64_t x) {   // splitmix64
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
struct Draw {
    uint64_t x;
    int operator()(int n) { x = mix(x); return (int)(x % (uint64_t)n); }
};

static void set_family(RouteShape &s, int family) {
    s.family = family;
    s.block = family == ROUTE_GENERIC ? 0 : family == ROUTE_BIG ? 1024 : s.P <= 256 ? 256 : 512;
    s.epw = family == ROUTE_WAVE ? 64 / s.P : 1;
}
static void set_shape_bools(RouteShape &s, unsigned b) {   // 9 bits
    s.no_full = b & 1; s.no_wide = b & 2; s.no_strided = b & 4; s.no_inl_stats = b & 8; s.ff_count = b & 16; s.stats_inl = b & 32; s.pow2_dt = b & 64;
    s.flags = ((b & 128) ? EV2G_FLAG_LOG_SOC : 0) | ((b & 256) ? EV2G_FLAG_LOG_CS_HISTORY : 0) | EV2G_FLAG_REFILLABLE;   // (a flag no route reads rides along)
    s.inl_shape_reason = s.stats_inl ? "" : kShapeReason;
}
static void set_call_bools(RouteCall &c, unsigned b) {   // 10 bits
    c.actions = b & 1; c.act32 = b & 2; c.obs = b & 4; c.obs32 = b & 8; c.reward = b & 16; c.done = b & 32; c.mask = b & 64;
    c.x_cost = b & 128; c.x_obs_f32 = b & 256; c.x_actions_f32 = b & 512;
}
static void set_strides(RouteCall &c, const int i[7]) {
    c.a_stride = kStrides[i[0]]; c.o_stride = kStrides[i[1]]; c.r_stride = kStrides[i[2]]; c.d_stride = kStrides[i[3]]; c.m_stride = kStrides[i[4]];
    c.x_cost_stride = kStrides[i[5]]; c.x_obs_f32_stride = kStrides[i[6]];
}

static void sweep_booleans(uint64_t salt) {
    g_case = "sweep 1: booleans x family x state kind";
    for (int fam : kFamilies)
        for (int sk = 0; sk < 3; sk++)
            for (unsigned sb = 0; sb < 512; sb++)
                for (unsigned cb = 0; cb < 1024; cb++) {
                    Draw d{salt ^ ((uint64_t)fam << 40) ^ ((uint64_t)sk << 36) ^ ((uint64_t)sb << 16) ^ cb};
                    RouteShape s;
                    s.T = kT; s.P = kPorts[d(7)]; s.D = 60 + d(2); s.npc = 1 + (d(4) == 0); s.state_kind = sk; s.reward_kind = kRewards[d(5)];
                    set_family(s, fam); set_shape_bools(s, sb);
                    RouteCall c;
                    set_call_bools(c, cb);
                    int si[7];
                    const bool plain = d(4) != 0;   // most points: strides that are not refused
                    for (int &v : si) v = plain ? d(2) : d(4);
                    set_strides(c, si);
                    const int tk = d(5);
                    c.t0 = kT0K[tk][0]; c.k = kT0K[tk][1]; c.auto_reset = d(3) == 0 ? d(3) : 0;
                    check_point(s, c);
                }
}

static void sweep_values() {
    g_case = "sweep 2: family x state kind x reward x P x auto_reset x (t0, k) x strides";
    for (int fam : kFamilies)
        for (int sk = 0; sk < 3; sk++)
            for (int rw : kRewards)
                for (int P : kPorts) {
                    RouteShape s;
                    s.T = kT; s.P = P; s.state_kind = sk; s.reward_kind = rw;
                    set_family(s, fam);
                    for (int ar = 0; ar < 3; ar++)
                        for (int tk = 0; tk < 5; tk++)
                            for (int half = 0; half < 2; half++)
                                for (int sv = 0; sv < (half ? 64 : 256); sv++) {
                                    Draw d{0x5eedull ^ ((uint64_t)fam << 50) ^ ((uint64_t)sk << 46) ^ ((uint64_t)rw << 40) ^ ((uint64_t)P << 32) ^ ((uint64_t)ar << 28) ^
                                           ((uint64_t)tk << 24) ^ ((uint64_t)half << 20) ^ (uint64_t)sv};
                                    s.D = 60 + d(2); s.npc = 1 + (d(4) == 0);
                                    // (the shape and call booleans: mostly the ones a specialisation needs, so that the values under sweep decide)
                                    unsigned sb = (unsigned)d(512), cb = (unsigned)d(1024);
                                    if (d(4) != 0) { sb = (sb & ~(1u | 2u | 4u | 8u | 256u)) | 16u | 32u | 64u | 128u; cb = (cb | 16u | 32u | 64u) & ~(128u | 256u); cb = d(2) ? ((cb | 1u | 4u)) : ((cb | 2u | 8u) & ~(1u | 4u)); }   // (one of the two pairs)
                                    set_shape_bools(s, sb);
                                    RouteCall c;
                                    set_call_bools(c, cb);
                                    int si[7];
                                    if (half == 0) { si[0] = d(2); si[1] = sv & 3; si[2] = sv >> 2 & 3; si[3] = sv >> 4 & 3; si[4] = sv >> 6 & 3; si[5] = d(2) ; si[6] = d(2); }
                                    else { si[0] = sv & 3; si[5] = sv >> 2 & 3; si[6] = sv >> 4 & 3; for (int j = 1; j < 5; j++) si[j] = d(2); }
                                    set_strides(c, si);
                                    c.t0 = kT0K[tk][0]; c.k = kT0K[tk][1]; c.auto_reset = ar;
                                    check_point(s, c);
                                }
                    for (unsigned sb = 0; sb < 512; sb++) {
                        set_shape_bools(s, sb);
                        for (int D = 60; D < 62; D++) { s.D = D; g_shape = s; check_fused(s); }
                        check_direct(s);
                    }
                }
}

// ---- named cases: what the GPU suite asserts of the shipped configurations ----
static RouteShape shipped(int family, int sk, int rk, int P) {
    RouteShape s;
    s.T = kT; s.P = P; s.D = 2 * P + 62; s.npc = 1; s.state_kind = sk; s.reward_kind = rk; s.flags = EV2G_FLAG_LOG_SOC; s.pow2_dt = true;
    set_family(s, family);
    s.ff_count = family == ROUTE_WAVE && s.epw == 1; s.stats_inl = s.ff_count; s.inl_shape_reason = s.stats_inl ? "" : kShapeReason;
    return s;
}
static RouteCall float64_call(int t0, int k, long long stride) {
    RouteCall c;
    c.actions = c.obs = c.reward = c.done = c.mask = true;
    c.a_stride = c.o_stride = c.r_stride = c.d_stride = c.m_stride = stride;
    c.t0 = t0; c.k = k;
    return c;
}
static StepRoute named(const char *name, const RouteShape &s, const RouteCall &c) { g_case = name; g_shape = s; g_call = c; return route_step(s, c); }

static void named_cases() {
    const RouteShape cfg2 = shipped(ROUTE_WAVE, EV2G_STATE_V2G_PROFIT_MAX_LOADS, 0, 50), cfg3 = shipped(ROUTE_WAVE, EV2G_STATE_PUBLIC_PST, 1, 20);
    StepRoute r = named("cfg2, stride 0", cfg2, float64_call(0, kT, 0));
    CHECK(r.specialisation == 2 && r.sk == 0 && r.rk == 0 && !r.io32 && r.fullk == 2 && r.ff && r.inl_stats && same(r.general_reason, "") && same(r.inl_reason, ""));
    r = named("cfg2, a mid-episode persistent launch", cfg2, float64_call(0, kT - 1, 0));
    CHECK(r.specialisation == 2 && r.ff && !r.inl_stats && same(r.inl_reason, kNotEnd));
    r = named("cfg2, per-step launches", cfg2, float64_call(kT - 1, 1, 0));
    CHECK(r.specialisation == 2 && !r.ff && !r.inl_stats && same(r.inl_reason, kSingle));
    r = named("cfg2, strided", cfg2, float64_call(0, kT, 400));
    CHECK(r.specialisation == 3 && r.fullk == 3 && !r.ff && !r.inl_stats && same(r.inl_reason, kNotTwo));
    {
        RouteShape s = cfg2; s.no_wide = true;
        r = named("cfg2, EV2G_NO_WIDE", s, float64_call(0, kT, 0));
        CHECK(r.specialisation == 1 && r.ff && !r.inl_stats);
        s = cfg2; s.no_strided = true;
        r = named("cfg2, EV2G_NO_STRIDED", s, float64_call(0, kT, 400));
        CHECK(r.specialisation == 0 && same(r.general_reason, kStrided));
        s = cfg2; s.no_full = true;
        r = named("cfg2, EV2G_NO_FULL", s, float64_call(0, kT, 0));
        CHECK(r.specialisation == 0 && same(r.general_reason, kNoFull) && !r.ff);
    }
    {
        RouteCall c = float64_call(0, kT, 0); c.x_cost = true;
        r = named("cfg2, a registered cost buffer", cfg2, c);
        CHECK(r.specialisation == 0 && r.fullk == 0 && same(r.general_reason, "a cost buffer is registered (ev2g_set_step_extras)"));
        c = float64_call(0, kT, 0); c.obs = false;
        r = named("cfg2, obs NULL", cfg2, c);
        CHECK(r.specialisation == 0 && same(r.general_reason, kNoPair));
        c = float64_call(0, kT, 0); c.auto_reset = EV2G_AUTO_RESET_NEXT;
        r = named("cfg2, auto_reset", cfg2, c);
        CHECK(r.specialisation == 0 && same(r.general_reason, "auto_reset"));
        c = RouteCall{}; c.act32 = c.obs32 = c.reward = c.done = c.mask = c.x_actions_f32 = c.x_obs_f32 = true; c.k = 1;
        r = named("cfg2, the float32 hand-over (ev2g_rollout)", cfg2, c);
        CHECK(r.specialisation == 2 && r.io32 && !r.ff && !r.inl_stats);
        c = float64_call(0, 1, 0); c.o_stride = -1;
        r = named("cfg2, a negative stride", cfg2, c);
        CHECK(same(r.refusal, kRefusal));
    }
    r = named("a run-time reward", shipped(ROUTE_WAVE, EV2G_STATE_V2G_PROFIT_MAX_LOADS, EV2G_REWARD_V2G_PROFITMAX, 50), float64_call(0, kT, 0));
    CHECK(r.specialisation == 0 && r.rk == 3 && r.fullk == 0 &&
          same(r.general_reason, "the reward function is one of the eight selected at run time (only the shipped configs' three are compiled in)"));
    for (int k = 1; k <= kT; k++) {
        r = named("cfg3 (PublicPST) never fast-forwards", cfg3, float64_call(0, k, 0));
        CHECK(r.specialisation == 2 && r.sk == 1 && r.rk == 1 && !r.ff);
        RouteShape one = shipped(ROUTE_WAVE, EV2G_STATE_PUBLIC_PST, 1, 40);
        r = named("PublicPST with one env per wavefront never fast-forwards", one, float64_call(0, k, 0));
        CHECK(one.ff_count && r.specialisation == 2 && !r.ff && r.inl_stats == (k == kT));
    }
    r = named("cfg4", shipped(ROUTE_BIG, EV2G_STATE_V2G_PROFIT_MAX_LOADS, 0, 1000), float64_call(0, kT, 0));
    CHECK(r.specialisation == 5 && r.family == ROUTE_BIG && same(r.general_reason, "") && same(r.inl_reason, kNotWave));
    r = named("cfg4, EV2G_NO_BIG", shipped(ROUTE_V2, EV2G_STATE_V2G_PROFIT_MAX_LOADS, 0, 1000), float64_call(0, kT, 0));
    CHECK(r.specialisation == 1 && r.family == ROUTE_V2 && r.spec);
    r = named("cfg4, strided", shipped(ROUTE_BIG, EV2G_STATE_V2G_PROFIT_MAX_LOADS, 0, 1000), float64_call(0, kT, 4000));
    CHECK(r.specialisation == 0 && r.family == ROUTE_V2 && r.block == 1024 && !r.spec);
    r = named("the generic kernel", shipped(ROUTE_GENERIC, EV2G_STATE_V2G_PROFIT_MAX_LOADS, 0, 2000), float64_call(0, kT, 0));
    CHECK(r.specialisation == -1 && r.family == ROUTE_GENERIC);
}

int main() {
    named_cases();
    sweep_booleans(1);
    sweep_booleans(2);
    sweep_values();
    g_case = "coverage";
    int n_wave = 0, n_fused = 0;
    for (int sk = 0; sk < 3; sk++)
        for (int rk = 0; rk < 4; rk++)
            for (int io32 = 0; io32 < 2; io32++)
                for (int fullk = 0; fullk < 4; fullk++) {
                    const bool seen = g_wave_seen[route_wave_index(sk, rk, io32 != 0, fullk)];
                    if (seen != route_wave_exists(sk, rk, io32 != 0, fullk)) { std::fprintf(stderr, "FAIL [coverage] ev2g_step_wave<%d, %d, %d, %d> %s\n", sk, rk, io32, fullk, seen ? "is routed to but does not exist" : "exists but no route reaches it"); return 1; }
                    n_wave += seen;
                }
    for (int i = 0; i < ROUTE_FUSED_ENTRIES; i++) {
        if (g_fused_hit[i] != route_fused_key(i).exists) { std::fprintf(stderr, "FAIL [coverage] fused entry %d\n", i); return 1; }
        n_fused += g_fused_hit[i];
    }
    if (n_wave != 69 || n_fused != 21) { std::fprintf(stderr, "FAIL [coverage] %d step instantiations (69), %d fused ones (21)\n", n_wave, n_fused); return 1; }   // 69 + 21 = the 90 of tests/test_abi_cpu.py
    std::printf("route_check: ok (%lld points)\n", g_points);
    return 0;
}
