// sac_check.cpp -- the SAC learner's host-only half (ev2gym_amd/csrc/ev2g_sac_host.h, ev2g_sac.h's element functions, the stacked-head index of
// ev2g_policy_host.h), without HIP:
//   a. plan_sac refuses every shape outside the stated limits with the message spelled out here, and sac_fields every bad config value, in table
//      order; the parameter blocks are laid out in SB3's order and the workspace's blocks neither overlap nor leave gaps;
//   b. writing the two heads element by element through sac_head_index (the loop of ev2g_sac_repack_kernel, one thread) reproduces
//      pack_linear_f32 of the stacked [2 n3, h2] matrix bit for bit, covers every element of both heads exactly once and touches no padding;
//      the trunk's images likewise through packed_f32_index;
//   c. the host twins of the element functions against their float64 forms.
//
//   c++ -std=c++17 -O1 -ffp-contract=off tests/host/sac_check.cpp -o sac_check && ./sac_check      (also with -fsanitize=address,undefined)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#define __host__
#define __device__
#include "../../ev2gym_amd/csrc/ev2g_sac_host.h"

static int fails = 0, checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

static uint64_t hash64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static float rnd(uint64_t i) { return (float)((double)(hash64(i) >> 11) / 9007199254740992.0 * 2.0 - 1.0); }

// ---- a. refusals and layouts ----
static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();
struct Field { const char *name; double ev2g_sac_config::*at; double bad[2]; int n_bad; double good; const char *tail; };
static const Field FIELDS[] = {
    {"lr", &ev2g_sac_config::lr, {-1e-9, 0}, 1, 0.0, ": lr must be finite and >= 0"},
    {"beta1", &ev2g_sac_config::beta1, {-0.1, 1.0}, 2, 0.0, ": beta1 must be in [0, 1)"},
    {"beta2", &ev2g_sac_config::beta2, {-0.1, 1.0}, 2, 0.0, ": beta2 must be in [0, 1)"},
    {"adam_eps", &ev2g_sac_config::adam_eps, {0.0, -1e-8}, 2, 1e-12, ": adam_eps must be finite and > 0"},
    {"tau", &ev2g_sac_config::tau, {-1e-9, 1.0000001}, 2, 1.0, ": tau must be in [0, 1]"},
    {"gamma", &ev2g_sac_config::gamma, {-1e-9, 1.0000001}, 2, 1.0, ": gamma must be in [0, 1]"},
    {"ent_coef", &ev2g_sac_config::ent_coef, {0.0, -0.1}, 2, 1e-3, ": ent_coef must be finite and > 0"},
};
static void check_refusals() {
    ev2g_sac_config def;
    sac_default_config(&def);
    CHECK(def.lr == 3e-4 && def.beta1 == 0.9 && def.beta2 == 0.999 && def.adam_eps == 1e-8 && def.tau == 0.005 && def.gamma == 0.99 && def.ent_coef == 1.0 &&
          def.n_critics == 2 && def.target_update_interval == 1 && def.ent_coef_auto == 1 && def.target_entropy_auto == 1, "SB3's defaults");
    CHECK(learner_refusal("who", sac_fields(def)).empty(), "the defaults are accepted");
    CHECK(sac_target_entropy(def, 20) == -20.0, "target_entropy auto is -P");
    const int n = (int)(sizeof(FIELDS) / sizeof(FIELDS[0]));
    for (int i = 0; i < n; i++) {
        const Field &f = FIELDS[i];
        const std::string want = std::string("who") + f.tail;
        double bad[5] = {NaN, Inf, -Inf, f.bad[0], f.bad[1]};
        for (int b = 0; b < 3 + f.n_bad; b++) {
            ev2g_sac_config c = def;
            c.*(f.at) = bad[b];
            CHECK(learner_refusal("who", sac_fields(c)) == want, "%s = %g: \"%s\"", f.name, bad[b], learner_refusal("who", sac_fields(c)).c_str());
            for (int j = i + 1; j < n; j++) {   // the earlier of two bad fields is the one named
                ev2g_sac_config c2 = c;
                c2.*(FIELDS[j].at) = NaN;
                CHECK(learner_refusal("who", sac_fields(c2)) == want, "%s and %s bad: the first is named", f.name, FIELDS[j].name);
            }
        }
        ev2g_sac_config c = def;
        c.*(f.at) = f.good;
        CHECK(learner_refusal("who", sac_fields(c)).empty(), "%s = %g is accepted", f.name, f.good);
    }
    for (double te : {NaN, Inf, -Inf}) {
        ev2g_sac_config c = def;
        c.target_entropy = te;
        CHECK(learner_refusal("who", sac_fields(c)).empty(), "target_entropy is not read under auto");
        c.target_entropy_auto = 0;
        CHECK(learner_refusal("who", sac_fields(c)) == "who: target_entropy must be finite and >= 0", "a target_entropy that is not finite");
    }
    {
        ev2g_sac_config c = def;
        c.target_entropy_auto = 0; c.target_entropy = -7.5;
        CHECK(learner_refusal("who", sac_fields(c)).empty() && sac_target_entropy(c, 20) == -7.5, "a negative target_entropy is accepted");
    }
    for (int tui : {0, -1}) {
        ev2g_sac_config c = def;
        c.target_update_interval = tui;
        CHECK(learner_refusal("who", sac_fields(c)) == "who: target_update_interval must be finite and >= 1", "target_update_interval %d", tui);
    }
    CHECK(learner_refusal("who", sac_rate_fields(NaN)) == "who: lr must be finite and >= 0" && learner_refusal("who", sac_rate_fields(0.0)).empty(), "the rate's list");

    struct { int d_in, h1, h2, d_out, nc; const char *msg; } shapes[] = {
        {0, 256, 256, 20, 2, "ev2g_sac: d_in 0 is outside 1 .. 192"}, {193, 256, 256, 20, 2, "ev2g_sac: d_in 193 is outside 1 .. 192"},
        {63, 0, 256, 20, 2, "ev2g_sac: h1 0 is outside 1 .. 256"}, {63, 257, 256, 20, 2, "ev2g_sac: h1 257 is outside 1 .. 256"},
        {63, 256, 0, 20, 2, "ev2g_sac: h2 0 is outside 1 .. 256"}, {63, 256, 257, 20, 2, "ev2g_sac: h2 257 is outside 1 .. 256"},
        {63, 256, 256, 0, 2, "ev2g_sac: d_out 0 is outside 1 .. 64"}, {63, 256, 256, 65, 2, "ev2g_sac: d_out 65 is outside 1 .. 64"},
        {63, 256, 256, 20, 0, "ev2g_sac: n_critics 0 is outside 1 .. 2"}, {63, 256, 256, 20, 3, "ev2g_sac: n_critics 3 is outside 1 .. 2"},
        {193, 257, 257, 65, 3, "ev2g_sac: d_in 193 is outside 1 .. 192"},
    };
    for (const auto &s : shapes) {
        const SacPlan p = plan_sac(s.d_in, s.h1, s.h2, s.d_out, s.nc);
        CHECK(p.err == EV2G_ERR_ARG && p.refusal == s.msg, "plan_sac(%d, %d, %d, %d, %d): \"%s\"", s.d_in, s.h1, s.h2, s.d_out, s.nc, p.refusal.c_str());
    }
    const int accepted[4][5] = {{192, 256, 256, 64, 2}, {1, 1, 1, 1, 1}, {63, 33, 17, 20, 2}, {162, 256, 256, 50, 1}};
    for (const auto &lim : accepted) {
        const SacPlan p = plan_sac(lim[0], lim[1], lim[2], lim[3], lim[4]);
        const int D = lim[0], h1 = lim[1], h2 = lim[2], P = lim[3], nc = lim[4], DA = D + P;
        CHECK(!p.err, "plan_sac accepts %d-%d-%d-%d x %d", D, h1, h2, P, nc);
        // SB3's order, no gaps: each array starts where the previous one of its size ends
        const int asz[8] = {h1 * D, h1, h2 * h1, h2, P * h2, P, P * h2, P}, csz[6] = {h1 * DA, h1, h2 * h1, h2, h2, 1};
        int o = 0;
        for (int i = 0; i < 8; i++) { CHECK(p.aoff[i] == o, "actor array %d at %d, expected %d", i, p.aoff[i], o); o += asz[i]; }
        CHECK(p.aoff[8] == o && p.n_actor == o, "the actor's block");
        CHECK(p.aoff[6] - p.aoff[4] == p.head_block && p.aoff[7] - p.aoff[5] == p.head_block, "the log_std head is one head_block behind mu's");
        o = 0;
        for (int i = 0; i < 6; i++) { CHECK(p.coff[i] == o, "critic array %d", i); o += csz[i]; }
        CHECK(p.coff[6] == o && p.n_critic == o && p.n_params == p.n_actor + nc * o && p.da == DA, "block sizes");
        CHECK(p.k1 % 8 == 0 && p.k1 >= D && p.k1 < D + 8 && p.n1 % 32 == 0 && p.n1 >= h1 && p.n1 < h1 + 32 && p.n2 % 32 == 0 && p.n2 >= h2 && p.n2 < h2 + 32 &&
              p.n3 % 32 == 0 && p.n3 >= P && p.n3 < P + 32, "padded widths");
        const long long R = EV2G_TD3_MAX_BATCH;
        const long long sizes[22] = {R * DA, R * DA, R * h1, R * h2, 2 * R * P, R * P, R * P, R, R, nc * R * h1, nc * R * h2, nc * R, nc * R, R, nc * R, nc * R * h2,
                                     nc * R * h1, nc * R * P, 2 * R * P, 2 * R * h2, R * h2, R * h1};
        const long long at[22] = {p.w_xa, p.w_xb, p.w_ah1, p.w_ah2, p.w_head, p.w_eps, p.w_a, p.w_lp, p.w_lp2, p.w_ch1, p.w_ch2, p.w_q, p.w_tq, p.w_y, p.w_dq, p.w_d2,
                                  p.w_d1, p.w_dxa, p.w_dhead, p.w_e2z, p.w_e2, p.w_e1};
        long long w = 0;
        for (int i = 0; i < 22; i++) { CHECK(at[i] == w, "workspace block %d at %lld, expected %lld", i, at[i], w); w += sizes[i]; }
        CHECK(p.w_floats == w, "workspace size");
        const SacDev d = sac_dev(p, 0.0f);
        CHECK(ev2g_sac_lds(d).bytes <= ev2g_sac_lds_max(), "LDS of %d-%d-%d-%d: %zu bytes", D, h1, h2, P, ev2g_sac_lds(d).bytes);
    }
    CHECK(ev2g_sac_lds(sac_dev(plan_sac(192, 256, 256, 64, 2), -1.0f)).bytes == 66560 && ev2g_sac_lds_max() == 66560, "the largest network's LDS");
}

// ---- b. the images ----
static void check_images(int D, int h1, int h2, int P) {
    const SacPlan p = plan_sac(D, h1, h2, P, 2);
    CHECK(!p.err, "plan");
    std::vector<float> W1((size_t)h1 * D), W2((size_t)h2 * h1), Wh[2], bh[2];
    for (size_t e = 0; e < W1.size(); e++) W1[e] = rnd(e + 1) + 2.0f;   // (never 0: a data position differs from the all-zero image)
    for (size_t e = 0; e < W2.size(); e++) W2[e] = rnd(e + 100003) + 2.0f;
    for (int hd = 0; hd < 2; hd++) {
        Wh[hd].resize((size_t)P * h2); bh[hd].resize((size_t)P);
        for (size_t e = 0; e < Wh[hd].size(); e++) Wh[hd][e] = rnd(e + 7000003ull * (uint64_t)(hd + 1)) + 2.0f;
        for (size_t e = 0; e < bh[hd].size(); e++) bh[hd][e] = rnd(e + 9000011ull * (uint64_t)(hd + 1)) + 2.0f;
    }
    // the stacked matrix [2 n3, h2]: head hd's rows at hd n3 .. hd n3 + P, zeros between
    std::vector<float> stacked((size_t)2 * p.n3 * h2, 0.f);
    for (int hd = 0; hd < 2; hd++) std::copy(Wh[hd].begin(), Wh[hd].end(), stacked.begin() + (size_t)hd * p.n3 * h2);
    const std::vector<float> want = pack_linear_f32(stacked.data(), 2 * p.n3, h2, 2 * p.n3, p.n2);
    size_t sizes[6];
    sac_image_sizes(p, sizes);
    CHECK(want.size() == sizes[4], "the stacked image's size");
    std::vector<float> got(sizes[4], 0.f), gotb(sizes[5], 0.f);
    std::vector<int> wrote(sizes[4], 0), wrote_b(sizes[5], 0);
    for (int hd = 0; hd < 2; hd++) {
        for (long long i = 0; i < (long long)P * h2; i++) {
            const size_t at = sac_head_index(hd, (int)(i / h2), (int)(i % h2), p.n3, p.n2);
            CHECK(at < got.size(), "head %d element %lld: index %zu outside the image", hd, i, at);
            if (at < got.size()) { got[at] = Wh[hd][(size_t)i]; wrote[at]++; }
        }
        for (int i = 0; i < P; i++) { gotb[(size_t)(hd * p.n3 + i)] = bh[hd][(size_t)i]; wrote_b[(size_t)(hd * p.n3 + i)]++; }
    }
    CHECK(std::memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0, "%d-%d-%d-%d: the stacked head image differs", D, h1, h2, P);
    long long once = 0, more = 0, pad_hit = 0;
    for (size_t i = 0; i < wrote.size(); i++) { once += wrote[i] == 1; more += wrote[i] > 1; pad_hit += wrote[i] > 0 && want[i] == 0.f; }
    CHECK(once == 2ll * P * h2 && more == 0 && pad_hit == 0, "head positions: %lld once (expected %lld), %lld more than once, %lld on padding", once, 2ll * P * h2, more, pad_hit);
    long long bw = 0;
    for (int c : wrote_b) { CHECK(c <= 1, "a bias position written twice"); bw += c; }
    CHECK(bw == 2 * P, "bias positions written: %lld", bw);
    for (int i = 0; i < 2 * p.n3; i++) CHECK((gotb[(size_t)i] != 0.f) == (i % p.n3 < P), "bias padding %d", i);
    // the trunk's two matrices through packed_f32_index
    const struct { const std::vector<float> *W; int n_out, n_in, N, K; } layers[2] = {{&W1, h1, D, p.n1, p.k1}, {&W2, h2, h1, p.n2, p.n1}};
    for (const auto &L : layers) {
        const std::vector<float> w = pack_linear_f32(L.W->data(), L.n_out, L.n_in, L.N, L.K);
        std::vector<float> g(w.size(), 0.f);
        std::vector<int> cnt(w.size(), 0);
        for (long long i = 0; i < (long long)L.n_out * L.n_in; i++) {
            const size_t at = packed_f32_index((int)(i / L.n_in), (int)(i % L.n_in), L.K);
            CHECK(at < g.size(), "trunk index outside the image");
            if (at < g.size()) { g[at] = (*L.W)[(size_t)i]; cnt[at]++; }
        }
        long long c1 = 0;
        for (int c : cnt) c1 += c == 1;
        CHECK(std::memcmp(g.data(), w.data(), w.size() * sizeof(float)) == 0 && c1 == (long long)L.n_out * L.n_in, "a trunk image differs");
    }
}

// ---- c. the host twins ----
static void check_twins() {
    const int B = 37, P = 13;
    std::vector<float> mu((size_t)B * P), ls((size_t)B * P), eps((size_t)B * P), g((size_t)B * P), a((size_t)B * P), ae((size_t)B * P), lp((size_t)B), dm((size_t)B * P),
        dl((size_t)B * P);
    for (size_t i = 0; i < mu.size(); i++) { mu[i] = rnd(i) * 2.5f; ls[i] = rnd(500 + i) * 13.0f - 10.0f; eps[i] = rnd(900 + i) * 3.0f; g[i] = rnd(1300 + i); }
    ls[0] = -20.0f; ls[1] = 2.0f; ls[2] = -25.0f; ls[3] = 3.0f;   // on and past both ends of the clamp
    const float la = (float)std::log(0.3);
    const double alpha = std::exp((double)la);
    sac_host_head(mu.data(), ls.data(), eps.data(), B, P, 0.0f, a.data(), ae.data(), lp.data());
    sac_host_head_back(mu.data(), ls.data(), eps.data(), g.data(), B, P, la, dm.data(), dl.data());
    int below = 0, above = 0;
    for (int b = 0; b < B; b++) {
        double sum = 0.0;
        for (int p = 0; p < P; p++) {
            const size_t i = (size_t)b * P + p;
            const double raw = ls[i], l = std::fmin(std::fmax(raw, -20.0), 2.0), e = eps[i], sg = std::exp(l), t = std::tanh((double)mu[i] + sg * e), omt = 1.0 - t * t;
            below += raw <= -20.0; above += raw >= 2.0;
            sum += -0.5 * e * e - l - 0.5 * std::log(2.0 * M_PI) - std::log(omt + 1e-6);
            CHECK(a[i] == (float)t && ae[i] == 0.5f * ((float)t + 1.0f), "a[%zu]", i);
            const double du = (alpha * 2.0 * t * omt / (omt + 1e-6) - (double)g[i] * omt) / B;
            const double dls = (raw > -20.0 && raw < 2.0) ? du * sg * e - alpha / B : 0.0;
            CHECK(std::fabs(dm[i] - du) <= 1.2e-7 * std::fabs(du) + 1e-45, "d_mu[%zu] %g vs %g", i, dm[i], du);
            CHECK(std::fabs(dl[i] - dls) <= 1.2e-7 * std::fabs(dls) + 1e-45 && (dls != 0.0 || dl[i] == 0.0f), "d_log_std[%zu] %g vs %g", i, dl[i], dls);
        }
        CHECK(std::fabs(lp[(size_t)b] - sum) <= 1.2e-7 * std::fabs(sum) + 1e-12 * P, "log pi[%d] %g vs %g", b, lp[(size_t)b], sum);
    }
    CHECK(below >= 2 && above >= 2, "both clamps act in the case (%d, %d)", below, above);
    CHECK(ev2g_sac_unscale_action(-0.5f, 0.0f) == 0.25f && ev2g_sac_unscale_action(-0.5f, -1.0f) == -0.5f &&
          ev2g_td3_scale_action(ev2g_sac_unscale_action(0.25f, 0.0f), 0.0f) == 0.25f, "unscale and its inverse");
    std::vector<float> tq((size_t)2 * B), r((size_t)B), y((size_t)B);
    std::vector<uint8_t> done((size_t)B);
    for (int i = 0; i < 2 * B; i++) tq[(size_t)i] = rnd(5000 + (uint64_t)i) * 9.0f;
    for (int i = 0; i < B; i++) { r[(size_t)i] = rnd(7000 + (uint64_t)i) * 4.0f; done[(size_t)i] = (uint8_t)(hash64(8000 + (uint64_t)i) & 1); }
    for (int n = 1; n <= 2; n++) {
        sac_host_y(tq.data(), lp.data(), r.data(), done.data(), B, n, 0.99, la, y.data());
        for (int b = 0; b < B; b++) {
            float qm = tq[(size_t)b];
            if (n == 2 && tq[(size_t)(B + b)] < qm) qm = tq[(size_t)(B + b)];
            const double want = (double)r[(size_t)b] + (done[(size_t)b] ? 0.0 : 0.99) * ((double)qm - alpha * (double)lp[(size_t)b]);
            CHECK(y[(size_t)b] == (float)want, "y[%d] with %d critics", b, n);
        }
    }
}

int main() {
    check_refusals();
    check_images(192, 256, 256, 64);
    check_images(63, 64, 64, 20);
    check_images(11, 33, 17, 5);
    check_images(162, 256, 256, 50);
    check_images(1, 1, 1, 1);
    check_twins();
    if (fails) { std::printf("sac_check: %d of %d checks FAILED\n", fails, checks); return 1; }
    std::printf("sac_check: ok (%d checks)\n", checks);
    return 0;
}
