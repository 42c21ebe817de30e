// ars_check.cpp -- the ARS learner's host-only half (ev2gym_amd/csrc/ev2g_ars_host.h), without HIP:
//   a. plan_ars lays theta out in parameters_to_vector order for both policy kinds, at the limits and at D = 1 with widths 1 / 33 / 256; writing
//      theta element by element through ars_image_index reproduces the layers' pack_linear_f32 images and padded biases one behind the other,
//      covers every element exactly once and touches no padding; the LDS plan stays within ev2g_sac_lds_max();
//   b. the row -> (candidate, tile) map covers every row of a population launch exactly once, under its own candidate, at R 1, 31, 32, 33, 65;
//   c. every refusal message of the plan and of the config;
//   d. the host twins: perturb's two roundings and draw indices, the returns' order, the update against a float64 restatement, ties to the lower
//      index, equal returns leaving theta's bits alone, NaN and infinite returns refused.
//
//   c++ -std=c++17 -O1 -ffp-contract=off tests/host/ars_check.cpp -o ars_check && ./ars_check      (also with -fsanitize=address,undefined)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#define __host__
#define __device__
#include "../../ev2gym_amd/csrc/ev2g_ars_host.h"

static int fails = 0, checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

static uint64_t hash64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static float rnd(uint64_t i) { return (float)((double)(hash64(i) >> 11) / 9007199254740992.0 * 2.0 - 1.0); }
static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

// ---- a. layouts and images ----
static void check_layout(int kind, int D, int h1, int h2, int P) {
    const ArsPlan p = plan_ars(kind, D, h1, h2, P, 8, 8);
    CHECK(!p.err, "plan_ars accepts kind %d %d-%d-%d-%d: %s", kind, D, h1, h2, P, p.refusal.c_str());
    const ArsLayout &L = p.lay;
    const ArsDev &d = p.dev;
    std::vector<float> want;   // the images one behind the other
    std::vector<float> theta;
    auto matrix = [&](int n_out, int n_in, int N, int K) {
        std::vector<float> W((size_t)n_out * n_in);
        for (size_t e = 0; e < W.size(); e++) W[e] = rnd(theta.size() + e) + 2.0f;   // (never 0: a data position differs from padding)
        theta.insert(theta.end(), W.begin(), W.end());
        const std::vector<float> img = pack_linear_f32(W.data(), n_out, n_in, N, K);
        want.insert(want.end(), img.begin(), img.end());
    };
    auto vec = [&](int n, int N, bool in_theta) {
        std::vector<float> b((size_t)N, 0.f);
        if (in_theta)
            for (int e = 0; e < n; e++) { b[(size_t)e] = rnd(theta.size() + 77) + 2.0f; theta.push_back(b[(size_t)e]); }
        want.insert(want.end(), b.begin(), b.end());
    };
    if (kind == EV2G_ARS_MLP) {
        CHECK(L.n_arrays == 6 && L.off[0] == 0 && L.off[1] == h1 * D && L.off[2] == L.off[1] + h1 && L.off[3] == L.off[2] + h2 * h1 && L.off[4] == L.off[3] + h2 &&
              L.off[5] == L.off[4] + P * h2 && L.off[6] == L.off[5] + P && L.n_params == L.off[6], "W1 | b1 | W2 | b2 | W3 | b3");
        matrix(h1, D, d.n1, d.k1); vec(h1, d.n1, true); matrix(h2, h1, d.n2, d.n1); vec(h2, d.n2, true); matrix(P, h2, d.n3, d.n2); vec(P, d.n3, true);
        CHECK(d.n1 % 32 == 0 && d.n1 >= h1 && d.n1 < h1 + 32 && d.n2 % 32 == 0 && d.n2 >= h2 && d.n2 < h2 + 32, "padded hidden widths");
    } else {
        CHECK(L.n_arrays == 1 && L.n_params == P * D && L.off[1] == P * D && d.n1 == 0 && d.n2 == 0, "W alone");
        matrix(P, D, d.n3, d.k1); vec(P, d.n3, false);
    }
    CHECK(d.k1 % 8 == 0 && d.k1 >= D && d.k1 < D + 8 && d.n3 % 32 == 0 && d.n3 >= P && d.n3 < P + 32, "padded widths");
    CHECK((long long)want.size() == d.stride && (long long)theta.size() == L.n_params, "stride %lld vs %zu, n_params %d vs %zu", d.stride, want.size(), L.n_params, theta.size());
    CHECK(d.stride % 4 == 0 && d.o_w1 % 4 == 0 && d.o_w2 % 4 == 0 && d.o_w3 % 4 == 0, "the matrices' images are 16-byte aligned");
    std::vector<float> got((size_t)d.stride, 0.f), back(theta.size(), 0.f);
    std::vector<int> wrote((size_t)d.stride, 0);
    for (int i = 0; i < L.n_params; i++) {
        const long long at = ars_image_index(L, i);
        CHECK(at >= 0 && at < d.stride, "element %d: index %lld outside the image", i, at);
        if (at >= 0 && at < d.stride) { got[(size_t)at] = theta[(size_t)i]; wrote[(size_t)at]++; }
    }
    long long once = 0, pad_hit = 0;
    for (size_t i = 0; i < wrote.size(); i++) { once += wrote[i] == 1; pad_hit += wrote[i] > 0 && want[i] == 0.f; }
    CHECK(std::memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0, "kind %d %d-%d-%d-%d: the image differs", kind, D, h1, h2, P);
    CHECK(once == L.n_params && pad_hit == 0, "positions: %lld once of %d, %lld on padding", once, L.n_params, pad_hit);
    std::vector<float> img2((size_t)d.stride, 0.f);
    ars_pack(L, theta.data(), img2.data());
    ars_unpack(L, img2.data(), back.data());
    CHECK(std::memcmp(back.data(), theta.data(), theta.size() * sizeof(float)) == 0 && std::memcmp(img2.data(), want.data(), want.size() * sizeof(float)) == 0, "pack -> unpack");
    CHECK(p.lds == ev2g_ars_lds(d).bytes && p.lds <= ev2g_sac_lds_max(), "LDS %zu of %zu", p.lds, ev2g_sac_lds_max());
    CHECK(p.image_bytes == (size_t)17 * d.stride * 4 && p.delta_bytes == (size_t)8 * L.n_params * 4 && p.total_bytes > p.image_bytes + p.delta_bytes, "byte budget");
}

// ---- b. the row map ----
static void check_rows(int R, int C) {
    const int tpc = ars_tiles_per_candidate(R);
    CHECK(tpc == (R + 31) / 32, "tiles per candidate");
    std::vector<int> seen((size_t)R * C, 0);
    for (int b = 0; b < C * tpc; b++) {
        const ArsTile t = ars_tile_of(b, R);
        CHECK(t.cand == b / tpc && t.row0 == (long long)t.cand * R + 32 * (b % tpc), "workgroup %d of R %d", b, R);
        CHECK(t.live >= 1 && t.live <= 32 && t.live == ((b % tpc) < tpc - 1 || R % 32 == 0 ? 32 : R % 32), "live rows %d of workgroup %d, R %d", t.live, b, R);
        for (int r = 0; r < t.live; r++) {
            const long long row = t.row0 + r;
            CHECK(row >= 0 && row < (long long)R * C && row / R == t.cand, "row %lld under candidate %d", row, t.cand);
            if (row >= 0 && row < (long long)R * C) seen[(size_t)row]++;
        }
    }
    for (int s : seen) CHECK(s == 1, "a row covered %d times at R %d", s, R);
}

// ---- c. refusals ----
static void check_refusals() {
    struct { int kind, D, h1, h2, P, nd, nt; const char *msg; } shapes[] = {
        {2, 63, 64, 64, 20, 8, 8, "ev2g_ars: kind must be EV2G_ARS_MLP or EV2G_ARS_LINEAR"},
        {0, 0, 64, 64, 20, 8, 8, "ev2g_ars: d_in 0 is outside 1 .. 192"}, {1, 193, 64, 64, 20, 8, 8, "ev2g_ars: d_in 193 is outside 1 .. 192"},
        {0, 63, 0, 64, 20, 8, 8, "ev2g_ars: h1 0 is outside 1 .. 256"}, {0, 63, 257, 64, 20, 8, 8, "ev2g_ars: h1 257 is outside 1 .. 256"},
        {0, 63, 64, 0, 20, 8, 8, "ev2g_ars: h2 0 is outside 1 .. 256"}, {0, 63, 64, 257, 20, 8, 8, "ev2g_ars: h2 257 is outside 1 .. 256"},
        {0, 63, 64, 64, 0, 8, 8, "ev2g_ars: d_out 0 is outside 1 .. 64"}, {1, 63, 0, 0, 65, 8, 8, "ev2g_ars: d_out 65 is outside 1 .. 64"},
        {0, 63, 64, 64, 20, 0, 1, "ev2g_ars: n_delta 0 is outside 1 .. 4096"}, {0, 63, 64, 64, 20, 4097, 1, "ev2g_ars: n_delta 4097 is outside 1 .. 4096"},
        {0, 63, 64, 64, 20, 8, 0, "ev2g_ars: n_top 0 is outside 1 .. n_delta (8)"}, {0, 63, 64, 64, 20, 8, 9, "ev2g_ars: n_top 9 is outside 1 .. n_delta (8)"},
    };
    for (const auto &s : shapes) {
        const ArsPlan p = plan_ars(s.kind, s.D, s.h1, s.h2, s.P, s.nd, s.nt);
        CHECK(p.err == EV2G_ERR_ARG && p.refusal == s.msg, "plan_ars: \"%s\" (expected \"%s\")", p.refusal.c_str(), s.msg);
    }
    CHECK(!plan_ars(EV2G_ARS_LINEAR, 63, 0, 999, 20, 4096, 1).err, "the linear policy does not read h1, h2; n_delta at its limit");
    ev2g_ars_config def;
    ars_default_config(&def);
    CHECK(def.learning_rate == 0.02 && def.delta_std == 0.05 && def.alive_bonus_offset == 0.0 && def.n_delta == 8 && def.n_top == 8, "sb3_contrib's defaults");
    CHECK(ars_config_refusal("who", def).empty(), "the defaults are accepted");
    auto with = [&](auto set) { ev2g_ars_config c = def; set(c); return ars_config_refusal("who", c); };
    for (double bad : {NaN, Inf, -Inf, -1e-9}) CHECK(with([&](ev2g_ars_config &c) { c.learning_rate = bad; }) == "who: learning_rate must be finite and >= 0", "learning_rate %g", bad);
    CHECK(with([](ev2g_ars_config &c) { c.learning_rate = 0.0; }).empty(), "learning_rate 0 is accepted");
    for (double bad : {NaN, Inf, -Inf, 0.0, -0.05}) CHECK(with([&](ev2g_ars_config &c) { c.delta_std = bad; }) == "who: delta_std must be finite and > 0", "delta_std %g", bad);
    for (double bad : {NaN, Inf, -Inf}) CHECK(with([&](ev2g_ars_config &c) { c.alive_bonus_offset = bad; }) == "who: alive_bonus_offset must be finite", "alive_bonus_offset %g", bad);
    CHECK(with([](ev2g_ars_config &c) { c.alive_bonus_offset = -3.5; }).empty(), "a negative alive_bonus_offset is accepted");
    CHECK(with([](ev2g_ars_config &c) { c.n_delta = 0; }) == "who: n_delta 0 is outside 1 .. 4096" && with([](ev2g_ars_config &c) { c.n_delta = 4097; }) == "who: n_delta 4097 is outside 1 .. 4096", "n_delta");
    CHECK(with([](ev2g_ars_config &c) { c.n_top = 0; }) == "who: n_top 0 is outside 1 .. n_delta (8)" && with([](ev2g_ars_config &c) { c.n_top = 9; }) == "who: n_top 9 is outside 1 .. n_delta (8)", "n_top");
    CHECK(with([](ev2g_ars_config &c) { c.learning_rate = NaN; c.delta_std = NaN; c.n_delta = 0; }) == "who: learning_rate must be finite and >= 0", "the first bad field is named");
    CHECK(ars_rows_refusal("who", "the env count", 48, 8).empty() && ars_rows_refusal("who", "the env count", 16, 8).empty(), "multiples of 2 n_delta");
    CHECK(ars_rows_refusal("who", "the env count", 40, 8) == "who: the env count 40 is not a positive multiple of 2 n_delta (16)" &&
          ars_rows_refusal("who", "n_rows", 0, 8) == "who: n_rows 0 is not a positive multiple of 2 n_delta (16)", "the rows' refusal");
}

// ---- d. the twins ----
static float fake_normal(uint64_t seed, uint64_t j) { return rnd(seed * 1000003ull + j) * 3.0f; }
static void check_twins() {
    const int nd = 5, n = 13;
    std::vector<float> theta((size_t)n), delta((size_t)nd * n), cand((size_t)2 * nd * n), d2((size_t)nd * n);
    for (int i = 0; i < n; i++) theta[(size_t)i] = rnd(40 + i);
    ars_host_perturb(theta.data(), nd, n, 0.05, 9, 3, delta.data(), cand.data(), fake_normal);
    const float s = (float)0.05;
    for (int k = 0; k < nd; k++)
        for (int i = 0; i < n; i++) {
            const float d = fake_normal(9, (uint64_t)((3 * nd + k) * n + i)), ds = d * s;
            CHECK(delta[(size_t)k * n + i] == d && cand[(size_t)k * n + i] == theta[(size_t)i] + ds && cand[(size_t)(nd + k) * n + i] == theta[(size_t)i] - ds, "perturb (%d, %d)", k, i);
        }
    ars_host_perturb(theta.data(), nd, n, 0.05, 9, 4, d2.data(), nullptr, fake_normal);
    CHECK(d2[0] == fake_normal(9, (uint64_t)(4 * nd * n)) && ars_delta_index(4, nd, n, 0, 0) == ars_delta_index(3, nd, n, nd - 1, n - 1) + 1, "iteration n + 1 continues the index range");

    // returns: two accumulated segments, t ascending per env; the candidates' envs ascending, then the alive bonus
    const int E = 12, C = 4, R = 3, k1 = 5, k2 = 4;
    std::vector<double> rew((size_t)(k1 + k2) * E), env((size_t)E, 0.0), ret((size_t)C), env1((size_t)E, 0.0);
    for (size_t i = 0; i < rew.size(); i++) rew[i] = (double)rnd(900 + i) * 1e3 + 1e-7 * (double)i;
    ars_host_returns(env.data(), rew.data(), k1, E, E, C, 0.0, 0, nullptr);
    ars_host_returns(env.data(), rew.data() + (size_t)k1 * E, k2, E, E, C, -0.25, k1 + k2, ret.data());
    ars_host_returns(env1.data(), rew.data(), k1 + k2, E, E, C, 0.0, 0, nullptr);
    for (int e = 0; e < E; e++) {
        double a = 0.0;
        for (int t = 0; t < k1 + k2; t++) a += rew[(size_t)t * E + e];
        CHECK(env[(size_t)e] == a && env1[(size_t)e] == a, "env %d: two segments are one", e);
    }
    for (int c = 0; c < C; c++) {
        double a = 0.0;
        for (int e = 0; e < R; e++) a += env[(size_t)c * R + e];
        CHECK(ret[(size_t)c] == a + -0.25 * (double)(R * (k1 + k2)), "candidate %d's return", c);
    }

    // update against a float64 restatement
    std::vector<double> r = {3.0, -1.0, 7.5, 2.0, 0.5, 1.0, 4.0, -2.0, 2.5, 0.25};
    for (int nt : {5, 3, 1}) {
        std::vector<float> th = theta;
        std::vector<int32_t> rank((size_t)nd);
        ev2g_ars_report rep{};
        ars_host_update(th.data(), delta.data(), r.data(), nd, nt, n, 0.02, rank.data(), &rep);
        const int want_rank[5] = {2, 1, 0, 3, 4};   // scores 3, 4, 7.5, 2.5, 0.5
        for (int k = 0; k < nd; k++) CHECK(rank[(size_t)k] == want_rank[k], "rank[%d] = %d", k, rank[(size_t)k]);
        const int order[5] = {2, 1, 0, 3, 4};
        double sum = 0.0, sq = 0.0;
        for (int h = 0; h < 2; h++) for (int j = 0; j < nt; j++) sum += r[(size_t)(h * nd + order[j])];
        const double mean = sum / (2 * nt);
        for (int h = 0; h < 2; h++) for (int j = 0; j < nt; j++) sq += (r[(size_t)(h * nd + order[j])] - mean) * (r[(size_t)(h * nd + order[j])] - mean);
        const double sigma = std::sqrt(sq / (2 * nt - 1)), step = 0.02 / (nt * sigma + 1e-6);
        CHECK(!rep.refused && rep.first_bad == -1 && rep.n_top == nt && rep.sigma_r == sigma && rep.step == step, "n_top %d: sigma %g step %g", nt, rep.sigma_r, rep.step);
        for (int i = 0; i < n; i++) {
            double acc = 0.0;
            for (int j = 0; j < nt; j++) acc += (r[(size_t)order[j]] - r[(size_t)(nd + order[j])]) * (double)delta[(size_t)order[j] * n + i];
            CHECK(th[(size_t)i] == (float)((double)theta[(size_t)i] + step * acc), "theta[%d] with n_top %d", i, nt);
        }
    }
    {   // ties break to the lower index; equal returns leave theta's bits alone; NaN and infinity are refused
        std::vector<float> th = theta;
        std::vector<int32_t> rank((size_t)nd);
        ev2g_ars_report rep{};
        std::vector<double> tie = {1.0, 5.0, 5.0, 0.0, 5.0, 5.0, 1.0, 2.0, 5.0, 3.0};   // scores 5, 5, 5, 5, 5
        ars_host_update(th.data(), delta.data(), tie.data(), nd, 2, n, 0.02, rank.data(), &rep);
        for (int k = 0; k < nd; k++) CHECK(rank[(size_t)k] == k, "tied scores keep the index order (rank[%d] = %d)", k, rank[(size_t)k]);
        th = theta;
        std::vector<double> same((size_t)2 * nd, 3.25);
        ars_host_update(th.data(), delta.data(), same.data(), nd, nd, n, 0.02, rank.data(), &rep);
        CHECK(!rep.refused && rep.sigma_r == 0.0 && rep.step == 0.02 / 1e-6 && std::memcmp(th.data(), theta.data(), th.size() * sizeof(float)) == 0, "equal returns");
        for (double bad : {NaN, Inf, -Inf}) {
            std::vector<double> rb = r;
            rb[7] = bad;
            th = theta;
            ars_host_update(th.data(), delta.data(), rb.data(), nd, nd, n, 0.02, rank.data(), &rep);
            CHECK(rep.refused == 1 && rep.first_bad == 7 && std::memcmp(th.data(), theta.data(), th.size() * sizeof(float)) == 0, "a return of %g is refused", bad);
            rb[2] = bad;
            ars_host_update(th.data(), delta.data(), rb.data(), nd, nd, n, 0.02, rank.data(), &rep);
            CHECK(rep.refused == 1 && rep.first_bad == 2, "the first bad candidate is named");
        }
    }
}

int main() {
    const int kinds[2] = {EV2G_ARS_MLP, EV2G_ARS_LINEAR};
    for (int kind : kinds) {
        check_layout(kind, 192, 256, 256, 64);
        check_layout(kind, 1, 1, 1, 1);
        check_layout(kind, 1, 33, 33, 1);
        check_layout(kind, 1, 256, 256, 1);
        check_layout(kind, 1, 1, 256, 33);
        check_layout(kind, 63, 64, 64, 20);
        check_layout(kind, 162, 33, 17, 50);
    }
    for (int R : {1, 31, 32, 33, 65})
        for (int C : {1, 2, 6}) check_rows(R, C);
    check_refusals();
    check_twins();
    if (fails) { std::printf("ars_check: %d of %d checks FAILED\n", fails, checks); return 1; }
    std::printf("ars_check: ok (%d checks)\n", checks);
    return 0;
}
