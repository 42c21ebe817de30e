// td3_check.cpp -- the TD3 / DDPG learner's host-only half (ev2gym_amd/csrc/ev2g_td3_host.h, ev2g_td3.h's element functions, the element map of
// ev2g_policy_host.h), without HIP:
//   a. for every packing plan_mlp can return -- bf16 / F32 / F32X3 on both shipped streaming shapes, a generic shape and the odd 33-17 -- writing
//      the masters element by element through mlp_image_map reproduces pack_mlp's images bit for bit, starting from the images of an
//      all-zero network; no padding word is written (a shadow counts the writes: every data position once, nothing else);
//   b. td3_fields refuses every bad value of every config field, in table order, with the message spelled out here; plan_td3 and
//      td3_batch_refusal refuse the shapes outside the stated limits and lay the parameter blocks out in SB3's order;
//   c. the host twins of the target, of Polyak and of the sampler's pick against plain restatements.
//
//   c++ -std=c++17 -O1 -ffp-contract=off tests/host/td3_check.cpp -o td3_check && ./td3_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#define __host__
#define __device__
#include "../../ev2gym_amd/csrc/ev2g_policy_host.h"
#include "../../ev2gym_amd/csrc/ev2g_td3_host.h"

static int fails = 0, checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

static uint64_t hash64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static float rnd(uint64_t i) { return (float)((double)(hash64(i) >> 11) / 9007199254740992.0 * 2.0 - 1.0) * 0.37f; }

// ---- a. the element map ----
static void check_map(int d_in, int h1, int h2, int d_out, int precision, int want_kind) {
    const MlpPlan p = plan_mlp(d_in, h1, h2, d_out, -1.0f, precision);
    CHECK(!p.err && p.kind == want_kind, "plan %d-%d-%d-%d precision %d: kind %d, expected %d", d_in, h1, h2, d_out, precision, p.kind, want_kind);
    const int n_out[3] = {h1, h2, d_out}, n_in[3] = {d_in, h1, h2};
    std::vector<float> W[3], b[3], Z[3], zb[3];
    for (int i = 0; i < 3; i++) {
        W[i].resize((size_t)n_out[i] * n_in[i]); b[i].resize((size_t)n_out[i]);
        for (size_t e = 0; e < W[i].size(); e++) W[i][e] = rnd(1000003ull * (uint64_t)(i + 1) + e);
        for (size_t e = 0; e < b[i].size(); e++) b[i][e] = rnd(77ull + 5000011ull * (uint64_t)(i + 1) + e);
        Z[i].assign(W[i].size(), 0.f); zb[i].assign(b[i].size(), 0.f);
    }
    const MlpImages want = pack_mlp(p, W[0].data(), b[0].data(), W[1].data(), b[1].data(), W[2].data(), b[2].data());
    // the images of an all-zero network have zeros everywhere: what a position holds there and not in `want` is data, everything else padding
    MlpImages got = pack_mlp(p, Z[0].data(), zb[0].data(), Z[1].data(), zb[1].data(), Z[2].data(), zb[2].data());
    const bool f32 = p.kind == MLP_KIND_F32;
    void *w[3];
    float *bias[3];
    std::vector<std::vector<int>> wrote(3), wrote_b(3);
    for (int i = 0; i < 3; i++) {
        w[i] = f32 ? (void *)got.w32[i].data() : (void *)got.w16[i].data();
        wrote[i].assign(f32 ? got.w32[i].size() : got.w16[i].size(), 0);
        bias[i] = got.bias[i].empty() ? got.bias[0].data() + got.bias_off[i] : got.bias[i].data();
    }
    for (int i = 0; i < 3; i++) wrote_b[i].assign(got.bias[i].size(), 0);
    const MlpImageMap mp = mlp_image_map(p, w, bias);
    std::vector<float> flat;
    for (int i = 0; i < 3; i++) { flat.insert(flat.end(), W[i].begin(), W[i].end()); flat.insert(flat.end(), b[i].begin(), b[i].end()); }
    // (the loop of ev2g_td3_refresh_kernel, one thread)
    for (int l = 0; l < 3; l++) {
        const MlpLayerMap &L = mp.layer[l];
        CHECK(L.n_out == n_out[l] && L.n_in == n_in[l], "layer %d: the map's shape", l);
        const float *Wm = flat.data() + L.w_off, *bm = flat.data() + L.b_off;
        for (long long e = 0; e < (long long)L.n_out * L.n_in; e++) {
            const int n = (int)(e / L.n_in), k = (int)(e % L.n_in);
            if (L.kind == MLP_IMG_F32) {
                const size_t at = mlp_image_index(L, n, k, 0);
                CHECK(at < wrote[l].size(), "layer %d (%d, %d): index %zu outside the image", l, n, k, at);
                ((float *)L.w)[at] = Wm[e]; wrote[l][at]++;
            } else {
                float r = Wm[e];
                for (int q = 0; q < L.nw; q++) {
                    const size_t at = mlp_image_index(L, n, k, q);
                    CHECK(at < wrote[l].size(), "layer %d (%d, %d) term %d: index %zu outside the image", l, n, k, q, at);
                    ((uint16_t *)L.w)[at] = ev2g_bf16_term(&r); wrote[l][at]++;
                }
            }
        }
        for (int e = 0; e < L.n_out; e++) {
            L.bias[e] = bm[e];
            const size_t at = (size_t)(L.bias + e - (got.bias[l].empty() ? got.bias[0].data() : got.bias[l].data()));
            wrote_b[got.bias[l].empty() ? 0 : l][at]++;
        }
    }
    for (int i = 0; i < 3; i++) {
        const size_t bytes = want.weight_bytes(i);
        CHECK(bytes == got.weight_bytes(i) && std::memcmp(want.weight(i), got.weight(i), bytes) == 0, "%d-%d-%d-%d precision %d: the weight image of layer %d differs",
              d_in, h1, h2, d_out, precision, i);
        CHECK(want.bias[i].size() == got.bias[i].size() && (want.bias[i].empty() || std::memcmp(want.bias[i].data(), got.bias[i].data(), want.bias[i].size() * 4) == 0),
              "%d-%d-%d-%d precision %d: the bias image of layer %d differs", d_in, h1, h2, d_out, precision, i);
        const long long terms = p.kind == MLP_KIND_S16 ? p.s16.nw : 1;
        long long once = 0, more = 0;
        for (int c : wrote[i]) { once += c == 1; more += c > 1; }
        CHECK(more == 0 && once == (long long)n_out[i] * n_in[i] * terms, "layer %d: %lld positions written once (expected %lld), %lld more than once", i, once,
              (long long)n_out[i] * n_in[i] * terms, more);
    }
    long long bias_written = 0;
    for (int i = 0; i < 3; i++)
        for (int c : wrote_b[i]) { CHECK(c <= 1, "a bias position written twice"); bias_written += c; }
    CHECK(bias_written == h1 + h2 + d_out, "bias positions written: %lld", bias_written);
}

// ---- b. refusals ----
static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();
struct Field { const char *name; double ev2g_td3_config::*at; double bad[2]; int n_bad; double good; const char *tail; };
static const Field FIELDS[] = {
    {"lr", &ev2g_td3_config::lr, {-1e-9, 0}, 1, 0.0, ": lr must be finite and >= 0"},
    {"beta1", &ev2g_td3_config::beta1, {-0.1, 1.0}, 2, 0.0, ": beta1 must be in [0, 1)"},
    {"beta2", &ev2g_td3_config::beta2, {-0.1, 1.0}, 2, 0.0, ": beta2 must be in [0, 1)"},
    {"adam_eps", &ev2g_td3_config::adam_eps, {0.0, -1e-8}, 2, 1e-12, ": adam_eps must be finite and > 0"},
    {"tau", &ev2g_td3_config::tau, {-1e-9, 1.0000001}, 2, 1.0, ": tau must be in [0, 1]"},
    {"gamma", &ev2g_td3_config::gamma, {-1e-9, 1.0000001}, 2, 1.0, ": gamma must be in [0, 1]"},
    {"target_policy_noise", &ev2g_td3_config::target_policy_noise, {-0.2, 0}, 1, 0.0, ": target_policy_noise must be finite and >= 0"},
    {"target_noise_clip", &ev2g_td3_config::target_noise_clip, {-0.5, 0}, 1, 0.0, ": target_noise_clip must be finite and >= 0"},
};
static void check_refusals() {
    ev2g_td3_config td3, ddpg;
    td3_default_config(0, &td3); td3_default_config(1, &ddpg);
    CHECK(td3.lr == 1e-3 && td3.beta1 == 0.9 && td3.beta2 == 0.999 && td3.adam_eps == 1e-8 && td3.tau == 0.005 && td3.gamma == 0.99 &&
          td3.target_policy_noise == 0.2 && td3.target_noise_clip == 0.5 && td3.n_critics == 2 && td3.policy_delay == 2, "TD3's preset");
    CHECK(ddpg.lr == 1e-3 && ddpg.adam_eps == 1e-8 && ddpg.tau == 0.005 && ddpg.gamma == 0.99 && ddpg.target_policy_noise == 0.0 && ddpg.n_critics == 1 &&
          ddpg.policy_delay == 1, "DDPG's preset");
    CHECK(learner_refusal("who", td3_fields(td3)).empty() && learner_refusal("who", td3_fields(ddpg)).empty(), "the presets are accepted");
    const int n = (int)(sizeof(FIELDS) / sizeof(FIELDS[0]));
    for (int i = 0; i < n; i++) {
        const Field &f = FIELDS[i];
        const std::string want = std::string("who") + f.tail;
        double bad[5] = {NaN, Inf, -Inf, f.bad[0], f.bad[1]};
        for (int b = 0; b < 3 + f.n_bad; b++) {
            ev2g_td3_config c = td3;
            c.*(f.at) = bad[b];
            CHECK(learner_refusal("who", td3_fields(c)) == want, "%s = %g: \"%s\"", f.name, bad[b], learner_refusal("who", td3_fields(c)).c_str());
            for (int j = i + 1; j < n; j++) {   // the earlier of two bad fields is the one named
                ev2g_td3_config c2 = c;
                c2.*(FIELDS[j].at) = NaN;
                CHECK(learner_refusal("who", td3_fields(c2)) == want, "%s and %s bad: the first is named", f.name, FIELDS[j].name);
            }
        }
        ev2g_td3_config c = td3;
        c.*(f.at) = f.good;
        CHECK(learner_refusal("who", td3_fields(c)).empty(), "%s = %g is accepted", f.name, f.good);
    }
    for (int delay : {0, -1}) {
        ev2g_td3_config c = td3;
        c.policy_delay = delay;
        CHECK(learner_refusal("who", td3_fields(c)) == "who: policy_delay must be finite and >= 1", "policy_delay %d", delay);
    }
    CHECK(learner_refusal("who", td3_rate_fields(NaN)) == "who: lr must be finite and >= 0" && learner_refusal("who", td3_rate_fields(0.0)).empty(), "the rate's list");

    struct { int d_in, h1, h2, d_out, nc; const char *msg; } shapes[] = {
        {0, 400, 300, 20, 2, "ev2g_td3: d_in 0 is outside 1 .. 192"}, {193, 400, 300, 20, 2, "ev2g_td3: d_in 193 is outside 1 .. 192"},
        {63, 0, 300, 20, 2, "ev2g_td3: h1 0 is outside 1 .. 400"}, {63, 401, 300, 20, 2, "ev2g_td3: h1 401 is outside 1 .. 400"},
        {63, 400, 0, 20, 2, "ev2g_td3: h2 0 is outside 1 .. 400"}, {63, 400, 401, 20, 2, "ev2g_td3: h2 401 is outside 1 .. 400"},
        {63, 400, 300, 0, 2, "ev2g_td3: d_out 0 is outside 1 .. 64"}, {63, 400, 300, 65, 2, "ev2g_td3: d_out 65 is outside 1 .. 64"},
        {63, 400, 300, 20, 0, "ev2g_td3: n_critics 0 is outside 1 .. 2"}, {63, 400, 300, 20, 3, "ev2g_td3: n_critics 3 is outside 1 .. 2"},
        {193, 401, 401, 65, 3, "ev2g_td3: d_in 193 is outside 1 .. 192"},
    };
    for (const auto &s : shapes) {
        const Td3Plan p = plan_td3(s.d_in, s.h1, s.h2, s.d_out, s.nc);
        CHECK(p.err == EV2G_ERR_ARG && p.refusal == s.msg, "plan_td3(%d, %d, %d, %d, %d): \"%s\"", s.d_in, s.h1, s.h2, s.d_out, s.nc, p.refusal.c_str());
    }
    const int accepted[3][5] = {{192, 400, 400, 64, 2}, {1, 1, 1, 1, 1}, {63, 33, 17, 20, 2}};
    for (const auto &lim : accepted) {
        const Td3Plan p = plan_td3(lim[0], lim[1], lim[2], lim[3], lim[4]);
        const int D = lim[0], h1 = lim[1], h2 = lim[2], P = lim[3], nc = lim[4];
        CHECK(!p.err, "plan_td3 accepts %d-%d-%d-%d x %d", D, h1, h2, P, nc);
        const int a[7] = {0, h1 * D, h1 * D + h1, h1 * D + h1 + h2 * h1, h1 * D + h1 + h2 * h1 + h2, h1 * D + h1 + h2 * h1 + h2 + P * h2, h1 * D + h1 + h2 * h1 + h2 + P * h2 + P};
        const int DA = D + P;
        const int c[7] = {0, h1 * DA, h1 * DA + h1, h1 * DA + h1 + h2 * h1, h1 * DA + h1 + h2 * h1 + h2, h1 * DA + h1 + h2 * h1 + h2 + h2, h1 * DA + h1 + h2 * h1 + h2 + h2 + 1};
        for (int i = 0; i < 7; i++) CHECK(p.aoff[i] == a[i] && p.coff[i] == c[i], "offsets %d", i);
        CHECK(p.n_actor == a[6] && p.n_critic == c[6] && p.n_params == a[6] + nc * c[6] && p.da == DA, "block sizes");
        // the workspace's blocks, in order, do not overlap: each starts where the previous one of the stated size ends
        const long long R = EV2G_TD3_MAX_BATCH;
        const long long sizes[16] = {R * DA, R * DA, R * h1, R * h2, R * P, nc * R * h1, nc * R * h2, nc * R, nc * R, R, nc * R, nc * R * h2, nc * R * h1, R * h2, R * h1, R * P};
        const long long at[16] = {p.w_xa, p.w_xb, p.w_ah1, p.w_ah2, p.w_amu, p.w_ch1, p.w_ch2, p.w_q, p.w_tq, p.w_y, p.w_dq, p.w_d2, p.w_d1, p.w_e2, p.w_e1, p.w_dmu};
        long long o = 0;
        for (int i = 0; i < 16; i++) { CHECK(at[i] == o, "workspace block %d at %lld, expected %lld", i, at[i], o); o += sizes[i]; }
        CHECK(p.w_floats == o, "workspace size");
    }
    CHECK(td3_batch_refusal("who", 0) == "who: B 0 is outside 1 .. 1024" && td3_batch_refusal("who", 1025) == "who: B 1025 is outside 1 .. 1024", "B outside the cap");
    CHECK(td3_batch_refusal("who", 1).empty() && td3_batch_refusal("who", 1024).empty() && EV2G_TD3_MAX_BATCH >= 1024, "B inside the cap");
}

// ---- c. the host twins ----
static void check_twins() {
    const int B = 37, P = 5, nc = 2;
    std::vector<float> at((size_t)B * P), nrm((size_t)B * P), out((size_t)B * P), tq((size_t)nc * B), r((size_t)B), y((size_t)B);
    std::vector<uint8_t> done((size_t)B);
    for (size_t i = 0; i < at.size(); i++) { at[i] = rnd(i) * 3.5f; nrm[i] = rnd(900 + i) * 12.0f; }
    for (int i = 0; i < nc * B; i++) tq[(size_t)i] = rnd(5000 + (uint64_t)i) * 9.0f;
    for (int i = 0; i < B; i++) { r[(size_t)i] = rnd(7000 + (uint64_t)i) * 4.0f; done[(size_t)i] = (uint8_t)(hash64(8000 + (uint64_t)i) & 1); }
    td3_host_smooth(at.data(), nrm.data(), (long long)B * P, 0.2, 0.5, out.data());
    int clipped_eps = 0, clipped_a = 0;
    for (size_t i = 0; i < at.size(); i++) {
        float eps = 0.2f * nrm[i];
        if (eps < -0.5f) { eps = -0.5f; clipped_eps++; }
        if (eps > 0.5f) { eps = 0.5f; clipped_eps++; }
        float a = at[i] + eps;
        if (a < -1.0f) { a = -1.0f; clipped_a++; }
        if (a > 1.0f) { a = 1.0f; clipped_a++; }
        CHECK(out[i] == a, "smoothed element %zu", i);
    }
    CHECK(clipped_eps > 10 && clipped_a > 10, "both clamps act in the case (%d, %d)", clipped_eps, clipped_a);
    td3_host_smooth(at.data(), nullptr, (long long)B * P, 0.0, 0.5, out.data());   // (sigma 0: the normals are not read)
    for (size_t i = 0; i < at.size(); i++) CHECK(out[i] == (at[i] < -1.0f ? -1.0f : at[i] > 1.0f ? 1.0f : at[i]), "unsmoothed element %zu", i);
    for (int n = 1; n <= nc; n++) {
        td3_host_y(tq.data(), r.data(), done.data(), B, n, 0.99, y.data());
        for (int b = 0; b < B; b++) {
            float qm = tq[(size_t)b];
            if (n == 2 && tq[(size_t)(B + b)] < qm) qm = tq[(size_t)(B + b)];
            const float nd = done[(size_t)b] ? 0.0f : 1.0f;
            CHECK(y[(size_t)b] == r[(size_t)b] + (nd * 0.99f) * qm, "y[%d] with %d critics", b, n);
        }
    }
    std::vector<float> t(at), p(nrm);
    td3_host_polyak(t.data(), p.data(), (long long)t.size(), 0.005);
    const float omt = (float)(1.0 - 0.005), tau = (float)0.005;
    for (size_t i = 0; i < t.size(); i++) { const float a = at[i] * omt, b = tau * nrm[i]; CHECK(t[i] == a + b, "polyak element %zu", i); }
    t = at;
    td3_host_polyak(t.data(), p.data(), (long long)t.size(), 1.0);
    for (size_t i = 0; i < t.size(); i++) CHECK(t[i] == at[i] * 0.0f + nrm[i], "tau 1 copies");
    // the sampler's pick and stream index
    CHECK(ev2g_replay_pick(0.0, 7) == 0 && ev2g_replay_pick(0.999999999, 7) == 6 && ev2g_replay_pick(1.0, 7) == 6 && ev2g_replay_pick(0.5, 1) == 0, "picks at the ends");
    for (int n : {1, 2, 12, 37}) {
        for (int i = 0; i < 1000; i++) {
            const double u = (double)(hash64(31 * (uint64_t)n + (uint64_t)i) >> 11) / 9007199254740992.0;
            const int k = ev2g_replay_pick(u, n);
            CHECK(k >= 0 && k < n && k == (int)std::floor(u * n), "pick(%g, %d) = %d", u, n, k);
        }
    }
    CHECK(ev2g_replay_stream_index(0, 0) == 0 && ev2g_replay_stream_index(0, 1) == 3 && ev2g_replay_stream_index(1, 0) == 3ull * EV2G_TD3_MAX_BATCH &&
          ev2g_replay_stream_index(2, 1023) + 3 == ev2g_replay_stream_index(3, 0), "a draw's rows do not share uniforms with the next draw's");
    CHECK(ev2g_td3_scale_action(0.25f, 0.0f) == -0.5f && ev2g_td3_scale_action(0.25f, -1.0f) == 0.25f && ev2g_td3_scale_action(1.0f, 0.0f) == 1.0f &&
          ev2g_td3_scale_action(0.0f, 0.0f) == -1.0f, "the stored action as the critic reads it");
}

int main() {
    // both shipped streaming shapes in every precision (S16 packing with 1, 2, 3 terms), a generic shape and an odd one in every precision
    // (bf16 fragments, float32 operands), the two fixed-kernel shapes next to the shipped ones
    const int precisions[3] = {EV2G_MLP_BF16, EV2G_MLP_F32, EV2G_MLP_F32X3};
    for (int pr : precisions) {
        check_map(162, 400, 300, 50, pr, MLP_KIND_S16);
        check_map(63, 400, 300, 20, pr, MLP_KIND_S16);
        check_map(63, 64, 64, 20, pr, pr == EV2G_MLP_BF16 ? MLP_KIND_ANY : MLP_KIND_F32);
        check_map(33, 33, 17, 33, pr, pr == EV2G_MLP_BF16 ? MLP_KIND_ANY : MLP_KIND_F32);
        check_map(5, 129, 7, 1, pr, MLP_KIND_S16);
    }
    check_map(162, 416, 320, 50, EV2G_MLP_BF16, MLP_KIND_FIXED);
    check_refusals();
    check_twins();
    if (fails) { std::printf("td3_check: %d of %d checks FAILED\n", fails, checks); return 1; }
    std::printf("td3_check: ok (%d checks)\n", checks);
    return 0;
}
