// stamp_rule_check.cpp -- which step launches carry launch stamps: route_step's StepRoute::stamps (ev2gym_amd/csrc/ev2g_route_host.h) against the one
// rule the kernel compiles its two stamp sites under, timing_wave_stamped (ev2gym_amd/csrc/ev2g_timing_host.h; ev2g_step_wave.h: STAMPED).  A route
// that says "stamps" for an instantiation without the sites opens a slot no kernel writes: its reading is -1.  Exits non-zero at the first failure.
//
//   c++ -std=c++17 -O1 tests/host/stamp_rule_check.cpp -o stamp_rule_check && ./stamp_rule_check
//
// (tests/test_launch_timing_cpu.py does exactly that, and once more with -fsanitize=address,undefined.)
//   * the rule itself: FULLK 2 and nothing else, and every (state, compiled-in reward, action format) has that instantiation;
//   * route_step over families x state kinds x rewards x P x flags x switches x buffers x strides x auto_reset x (t0, k): stamps is never set for a
//     refused launch or outside ev2g_step_wave, and on it equals timing_wave_stamped(fullk) -- which is "ev2g_last_launch_specialisation == 2";
//   * witnesses: the benchmark's whole-episode call, a 1-step and a mid-episode call are stamped; strided outputs (3), a narrow env (1), a cost
//     buffer (0) and auto_reset (0) are not.
#include <cstdio>
#include <cstdlib>

#include "../../ev2gym_amd/csrc/ev2g_route_host.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL line %d: %s (%s; point %d %d %d %d %d %lld %d %d)\n", __LINE__, #cond, g_case, g_pt[0], g_pt[1], g_pt[2], g_pt[3], g_pt[4], g_os, g_pt[5], g_pt[6]); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)
static char g_case[256] = "";
static int g_pt[7];       // family, state kind, reward, P, bits, t0, k of the route in work
static long long g_os;    // its observation stride

static_assert(timing_wave_stamped(2) && !timing_wave_stamped(0) && !timing_wave_stamped(1) && !timing_wave_stamped(3) && !timing_wave_stamped(-1) &&
              !timing_wave_stamped(4), "the stamp sites live in the FULLK 2 instantiations only");

static RouteShape wave_shape(int sk, int rk, int P, int T) {
    RouteShape s;
    s.family = ROUTE_WAVE; s.P = P; s.T = T; s.D = 22 + 2 * P; s.npc = 1; s.state_kind = sk; s.reward_kind = rk; s.flags = EV2G_FLAG_LOG_SOC;
    s.epw = 64 / P > 0 ? 64 / P : 1; s.ff_count = s.epw == 1; s.stats_inl = s.epw == 1; s.balance = s.ff_count;
    return s;
}
static RouteCall full_call(int t0, int k) {
    RouteCall c;
    c.actions = c.obs = c.reward = c.done = c.mask = true; c.a_stride = 1; c.t0 = t0; c.k = k;
    return c;
}

int main() {
    const int T = 112;
    // every compiled-in reward has the stamped instantiation, in both action formats
    for (int sk = 0; sk < 3; sk++)
        for (int rk = 0; rk < 3; rk++) CHECK(route_wave_exists(sk, rk, false, 2) && route_wave_exists(sk, rk, true, 2));

    long long points = 0, stamped = 0;
    std::snprintf(g_case, sizeof g_case, "sweep");
    const int families[] = {ROUTE_GENERIC, ROUTE_V2, ROUTE_BIG, ROUTE_WAVE};
    const int Ps[] = {3, 10, 30, 50};
    const int rewards[] = {0, 1, 2, 3, 7};
    const long long strides[] = {0, 5, 1ll << 29};
    const int tk[][2] = {{0, 1}, {0, T}, {3, 5}, {T - 1, 1}, {T - 2, 2}, {T - 1, 2}};
    for (int fam : families)
        for (int sk = 0; sk < 3; sk++)
            for (int rw : rewards)
                for (int P : Ps)
                    for (int bits = 0; bits < (1 << 13); bits++)
                        for (long long os : strides)
                            for (const auto &w : tk) {
                                RouteShape s = wave_shape(sk, rw, P, T);
                                s.family = fam; s.block = fam == ROUTE_WAVE || fam == ROUTE_GENERIC ? 0 : 256; s.pow2_dt = true;
                                s.flags = ((bits & 1) ? EV2G_FLAG_LOG_SOC : 0) | ((bits & 2) ? EV2G_FLAG_LOG_CS_HISTORY : 0);
                                s.no_full = bits & 4; s.no_wide = bits & 8; s.no_strided = bits & 16;
                                RouteCall c;
                                c.actions = bits & 32; c.act32 = bits & 64; c.obs = bits & 128; c.obs32 = bits & 256;
                                c.reward = c.done = !(bits & 512); c.mask = true;
                                c.x_cost = bits & 1024; c.x_obs_f32 = bits & 2048; c.auto_reset = (bits & 4096) ? 1 : 0;
                                c.a_stride = 7; c.o_stride = os; c.t0 = w[0]; c.k = w[1];
                                g_pt[0] = fam; g_pt[1] = sk; g_pt[2] = rw; g_pt[3] = P; g_pt[4] = bits; g_pt[5] = w[0]; g_pt[6] = w[1]; g_os = os;
                                const StepRoute r = route_step(s, c);
                                points++;
                                if (r.refusal) { CHECK(!r.stamps); continue; }
                                if (r.family != ROUTE_WAVE) { CHECK(!r.stamps); continue; }
                                CHECK(r.stamps == timing_wave_stamped(r.fullk));
                                CHECK(r.stamps == (r.specialisation == 2));
                                if (r.stamps) { CHECK(route_wave_exists(r.sk, r.rk, r.io32, r.fullk) && os == 0); stamped++; }
                            }
    CHECK(stamped > 0 && stamped < points);

    // witnesses
    std::snprintf(g_case, sizeof g_case, "witnesses");
    const RouteShape head = wave_shape(EV2G_STATE_V2G_PROFIT_MAX_LOADS, 0, 50, T), pst = wave_shape(EV2G_STATE_PUBLIC_PST, 1, 20, T);
    CHECK(route_step(head, full_call(0, T)).stamps && route_step(pst, full_call(0, T)).stamps);   // the benchmark's launches, cfg2 and cfg3
    CHECK(route_step(head, full_call(0, 1)).stamps && route_step(head, full_call(3, 5)).stamps);
    RouteCall c = full_call(0, T);
    c.o_stride = 122; c.r_stride = 1; c.d_stride = 1; c.m_stride = 50;
    CHECK(route_step(head, c).fullk == 3 && !route_step(head, c).stamps);                           // every output kept
    CHECK(route_step(wave_shape(EV2G_STATE_V2G_PROFIT_MAX_LOADS, 0, 3, T), full_call(0, T)).fullk == 1 &&
          !route_step(wave_shape(EV2G_STATE_V2G_PROFIT_MAX_LOADS, 0, 3, T), full_call(0, T)).stamps);   // a narrow env
    c = full_call(0, T); c.x_cost = true;
    CHECK(route_step(head, c).fullk == 0 && !route_step(head, c).stamps);
    c = full_call(0, T); c.auto_reset = 1;
    CHECK(route_step(head, c).fullk == 0 && !route_step(head, c).stamps);
    std::printf("stamp_rule_check: ok (%lld routes, %lld stamped)\n", points, stamped);
    return 0;
}
