// tqc_check.cpp -- the TQC learner's host-only half (ev2gym_amd/csrc/ev2g_tqc_host.h, ev2g_tqc.h's element functions), without HIP:
//   a. plan_tqc refuses every shape and quantile setting outside the stated limits with the message spelled out here, the first bad field named;
//      every accepted (n_critics, n_quantiles, drop) has K = n_critics (n_quantiles - drop); the parameter blocks are in sb3_contrib's order; no
//      workspace block overlaps another, and the float64 partials sit on an even offset; the config's defaults and checks are SAC's;
//   b. the host sort (tqc_host_sort_row, the key of ev2g_tqc_key_less) against std::stable_sort under `<` on crafted rows -- all equal, reversed,
//      already sorted, ties across critics, +0 / -0 -- bit for bit, for M in {1, 2, 63, 64, 65, 127, 128}; the bitonic network of
//      ev2g_tqc_target_kernel, walked by one thread, leaves the same order;
//   c. the host twins of the target and of the critic head against their float64 forms.
//
//   c++ -std=c++17 -O1 -ffp-contract=off tests/host/tqc_check.cpp -o tqc_check && ./tqc_check      (also with -fsanitize=address,undefined)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#define __host__
#define __device__
#include "../../ev2gym_amd/csrc/ev2g_tqc_host.h"

static int fails = 0, checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

static uint64_t hash64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static float rnd(uint64_t i) { return (float)((double)(hash64(i) >> 11) / 9007199254740992.0 * 2.0 - 1.0); }
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// ---- a. refusals and layouts ----
static void check_plan() {
    struct { int d_in, h1, h2, d_out, nc, nq, drop; const char *msg; } shapes[] = {
        {0, 256, 256, 20, 2, 25, 2, "ev2g_tqc: d_in 0 is outside 1 .. 192"}, {193, 256, 256, 20, 2, 25, 2, "ev2g_tqc: d_in 193 is outside 1 .. 192"},
        {63, 0, 256, 20, 2, 25, 2, "ev2g_tqc: h1 0 is outside 1 .. 256"}, {63, 257, 256, 20, 2, 25, 2, "ev2g_tqc: h1 257 is outside 1 .. 256"},
        {63, 256, 0, 20, 2, 25, 2, "ev2g_tqc: h2 0 is outside 1 .. 256"}, {63, 256, 257, 20, 2, 25, 2, "ev2g_tqc: h2 257 is outside 1 .. 256"},
        {63, 256, 256, 0, 2, 25, 2, "ev2g_tqc: d_out 0 is outside 1 .. 64"}, {63, 256, 256, 65, 2, 25, 2, "ev2g_tqc: d_out 65 is outside 1 .. 64"},
        {63, 256, 256, 20, 0, 25, 2, "ev2g_tqc: n_critics 0 is outside 1 .. 5"}, {63, 256, 256, 20, 6, 25, 2, "ev2g_tqc: n_critics 6 is outside 1 .. 5"},
        {63, 256, 256, 20, 2, 0, 0, "ev2g_tqc: n_quantiles 0 is outside 1 .. 64"}, {63, 256, 256, 20, 2, 65, 2, "ev2g_tqc: n_quantiles 65 is outside 1 .. 64"},
        {63, 256, 256, 20, 3, 43, 2, "ev2g_tqc: n_critics * n_quantiles 129 is outside 1 .. 128"},
        {63, 256, 256, 20, 5, 26, 2, "ev2g_tqc: n_critics * n_quantiles 130 is outside 1 .. 128"},
        {63, 256, 256, 20, 2, 25, -1, "ev2g_tqc: top_quantiles_to_drop_per_net -1 is outside 0 .. 24"},
        {63, 256, 256, 20, 2, 25, 25, "ev2g_tqc: top_quantiles_to_drop_per_net 25 is outside 0 .. 24"},
        {63, 256, 256, 20, 1, 1, 1, "ev2g_tqc: top_quantiles_to_drop_per_net 1 is outside 0 .. 0"},
        {193, 257, 257, 65, 6, 65, 99, "ev2g_tqc: d_in 193 is outside 1 .. 192"},       // the first bad field is the one named
        {63, 256, 256, 20, 6, 65, 99, "ev2g_tqc: n_critics 6 is outside 1 .. 5"},
        {63, 256, 256, 20, 5, 65, 99, "ev2g_tqc: n_quantiles 65 is outside 1 .. 64"},
        {63, 256, 256, 20, 5, 64, 99, "ev2g_tqc: n_critics * n_quantiles 320 is outside 1 .. 128"},
    };
    for (const auto &s : shapes) {
        const TqcPlan p = plan_tqc(s.d_in, s.h1, s.h2, s.d_out, s.nc, s.nq, s.drop);
        CHECK(p.err == EV2G_ERR_ARG && p.refusal == s.msg, "plan_tqc(%d, %d, %d, %d, %d, %d, %d): \"%s\"", s.d_in, s.h1, s.h2, s.d_out, s.nc, s.nq, s.drop, p.refusal.c_str());
    }
    // every (nc, nq, drop): accepted exactly inside the limits, with K = nc (nq - drop)
    int accepted = 0;
    for (int nc = 0; nc <= 6; nc++)
        for (int nq = 0; nq <= 65; nq++)
            for (int drop = -1; drop <= nq + 1; drop++) {
                const TqcPlan p = plan_tqc(11, 33, 17, 5, nc, nq, drop);
                const bool ok = nc >= 1 && nc <= 5 && nq >= 1 && nq <= 64 && nc * nq <= 128 && drop >= 0 && drop <= nq - 1;
                CHECK((p.err == EV2G_OK) == ok, "plan_tqc(%d x %d, drop %d): err %d", nc, nq, drop, p.err);
                if (!p.err) { accepted++; CHECK(p.M == nc * nq && p.K == nc * (nq - drop) && p.K >= 1 && p.K <= p.M && p.nq == nq && p.drop == drop && p.nc == nc, "K of %d x %d drop %d", nc, nq, drop); }
            }
    CHECK(accepted > 1000, "accepted settings: %d", accepted);
    const int nets[5][7] = {{192, 256, 256, 64, 5, 25, 2}, {192, 256, 256, 64, 2, 64, 0}, {1, 1, 1, 1, 1, 1, 0}, {63, 33, 17, 20, 3, 7, 1}, {162, 256, 256, 50, 2, 25, 2}};
    for (const auto &lim : nets) {
        const int D = lim[0], h1 = lim[1], h2 = lim[2], P = lim[3], nc = lim[4], nq = lim[5], DA = D + P;
        const TqcPlan p = plan_tqc(D, h1, h2, P, nc, nq, lim[6]);
        CHECK(!p.err, "plan_tqc accepts %d-%d-%d-%d, %d x %d", D, h1, h2, P, nc, nq);
        const int asz[8] = {h1 * D, h1, h2 * h1, h2, P * h2, P, P * h2, P}, csz[6] = {h1 * DA, h1, h2 * h1, h2, nq * h2, nq};
        int o = 0;
        for (int i = 0; i < 8; i++) { CHECK(p.aoff[i] == o, "actor array %d at %d, expected %d", i, p.aoff[i], o); o += asz[i]; }
        CHECK(p.aoff[8] == o && p.n_actor == o, "the actor's block");
        o = 0;
        for (int i = 0; i < 6; i++) { CHECK(p.coff[i] == o, "critic array %d", i); o += csz[i]; }
        CHECK(p.coff[6] == o && p.n_critic == o && p.n_params == p.n_actor + nc * o && p.da == DA, "block sizes");
        // the actor side is SAC's: the same arrays and padded widths as plan_sac's of the same network
        const SacPlan sp = plan_sac(D, h1, h2, P, 1);
        CHECK(std::memcmp(sp.aoff, p.aoff, sizeof(sp.aoff)) == 0 && sp.head_block == p.head_block && sp.k1 == p.k1 && sp.n1 == p.n1 && sp.n2 == p.n2 && sp.n3 == p.n3,
              "the actor's layout is SAC's");
        const long long R = EV2G_TD3_MAX_BATCH;
        struct Block { long long at, size; const char *name; } blocks[] = {
            {p.w_xa, R * DA, "xa"}, {p.w_xb, R * DA, "xb"}, {p.w_ah1, R * h1, "ah1"}, {p.w_ah2, R * h2, "ah2"}, {p.w_head, 2 * R * P, "head"}, {p.w_eps, R * P, "eps"},
            {p.w_a, R * P, "a"}, {p.w_lp, R, "lp"}, {p.w_lp2, R, "lp2"}, {p.w_ch1, nc * R * h1, "ch1"}, {p.w_ch2, nc * R * h2, "ch2"}, {p.w_q, nc * R * nq, "q"},
            {p.w_tq, nc * R * nq, "tq"}, {p.w_dq, nc * R * nq, "dq"}, {p.w_d2, nc * R * h2, "d2"}, {p.w_d1, nc * R * h1, "d1"}, {p.w_dxa, nc * R * P, "dxa"},
            {p.w_dhead, 2 * R * P, "dhead"}, {p.w_e2z, 2 * R * h2, "e2z"}, {p.w_e2, R * h2, "e2"}, {p.w_e1, R * h1, "e1"}, {p.w_z, R * p.K, "z"},
            {p.w_part, 2 * R, "part"}, {p.w_g, R * P, "g"}};
        const int nb = (int)(sizeof(blocks) / sizeof(blocks[0]));
        for (int i = 0; i < nb; i++) {
            CHECK(blocks[i].at >= 0 && blocks[i].at + blocks[i].size <= p.w_floats, "block %s outside the workspace", blocks[i].name);
            for (int j = i + 1; j < nb; j++)
                CHECK(blocks[i].at + blocks[i].size <= blocks[j].at || blocks[j].at + blocks[j].size <= blocks[i].at, "blocks %s and %s overlap", blocks[i].name, blocks[j].name);
        }
        CHECK(p.w_part % 2 == 0, "the float64 partials at an odd float offset %lld", p.w_part);
    }
    ev2g_tqc_config def;
    tqc_default_config(&def);
    CHECK(def.lr == 3e-4 && def.beta1 == 0.9 && def.beta2 == 0.999 && def.adam_eps == 1e-8 && def.tau == 0.005 && def.gamma == 0.99 && def.ent_coef == 1.0 &&
          def.n_critics == 2 && def.target_update_interval == 1 && def.ent_coef_auto == 1 && def.target_entropy_auto == 1 && def.n_quantiles == 25 &&
          def.top_quantiles_to_drop_per_net == 2, "sb3_contrib's defaults");
    CHECK(learner_refusal("who", tqc_fields(def)).empty(), "the defaults are accepted");
    {
        ev2g_tqc_config c = def;
        c.tau = 1.5;
        CHECK(learner_refusal("who", tqc_fields(c)) == "who: tau must be in [0, 1]", "tau 1.5");
        c = def; c.ent_coef = 0.0;
        CHECK(learner_refusal("who", tqc_fields(c)) == "who: ent_coef must be finite and > 0", "ent_coef 0");
        c = def; c.target_update_interval = 0;
        CHECK(learner_refusal("who", tqc_fields(c)) == "who: target_update_interval must be finite and >= 1", "target_update_interval 0");
        c = def; c.lr = -1.0; c.gamma = 2.0;
        CHECK(learner_refusal("who", tqc_fields(c)) == "who: lr must be finite and >= 0", "the first bad field is named");
        const ev2g_sac_config s = tqc_sac_config(def);
        CHECK(s.lr == def.lr && s.tau == def.tau && s.gamma == def.gamma && s.n_critics == 2 && s.ent_coef_auto == 1 && s.target_entropy_auto == 1 &&
              sac_target_entropy(s, 20) == -20.0, "the shared fields");
    }
}

// ---- b. the sort ----
// the network of ev2g_tqc_target_kernel walked by one thread: 128 slots, slots past M hold (+inf, slot)
static void network_sort(const float *v, int M, float *out_v, int *out_i) {
    float kv[EV2G_TQC_MAX_ATOMS];
    int ki[EV2G_TQC_MAX_ATOMS];
    for (int m = 0; m < EV2G_TQC_MAX_ATOMS; m++) { kv[m] = m < M ? v[m] : std::numeric_limits<float>::infinity(); ki[m] = m; }
    for (int k = 2; k <= EV2G_TQC_MAX_ATOMS; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
            for (int t = 0; t < 64; t++) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                CHECK(lo >= 0 && lo < hi && hi < EV2G_TQC_MAX_ATOMS, "pair (%d, %d) of lane %d at k %d j %d", lo, hi, t, k, j);
                const bool up = (lo & k) == 0;
                if (ev2g_tqc_key_less(kv[hi], ki[hi], kv[lo], ki[lo]) == up) { std::swap(kv[lo], kv[hi]); std::swap(ki[lo], ki[hi]); }
            }
    for (int m = 0; m < EV2G_TQC_MAX_ATOMS; m++) { out_v[m] = kv[m]; out_i[m] = ki[m]; }
}
static void check_sort() {
    const int Ms[7] = {1, 2, 63, 64, 65, 127, 128};
    const char *kinds[7] = {"random", "equal", "reversed", "sorted", "ties across critics", "+0 / -0", "+inf atoms"};
    for (int M : Ms)
        for (int kind = 0; kind < 7; kind++)
            for (int rep = 0; rep < 3; rep++) {
                std::vector<float> v((size_t)M);
                const uint64_t base = (uint64_t)M * 1000003ull + (uint64_t)kind * 7919ull + (uint64_t)rep * 104729ull;
                for (int m = 0; m < M; m++) v[(size_t)m] = rnd(base + (uint64_t)m) * 5.0f;
                if (kind == 1) std::fill(v.begin(), v.end(), v[0]);
                if (kind == 2) std::sort(v.begin(), v.end(), [](float a, float b) { return a > b; });
                if (kind == 3) std::sort(v.begin(), v.end());
                if (kind == 4) { const int nq = M > 2 ? (M + 1) / 2 : 1; for (int m = nq; m < M; m++) v[(size_t)m] = v[(size_t)(m - nq)]; }   // critic 1 repeats critic 0
                if (kind == 5) for (int m = 0; m < M; m++) v[(size_t)m] = (hash64(base + 99 + (uint64_t)m) % 3 == 0) ? v[(size_t)m] : ((m & 1) ? -0.0f : 0.0f);
                if (kind == 6) for (int m = 0; m < M; m += 3) v[(size_t)m] = std::numeric_limits<float>::infinity();
                std::vector<int> want((size_t)M);
                for (int m = 0; m < M; m++) want[(size_t)m] = m;
                std::stable_sort(want.begin(), want.end(), [&v](int a, int b) { return v[(size_t)a] < v[(size_t)b]; });
                for (int K : {M, M > 4 ? M - 4 : 1, 1}) {
                    std::vector<float> got((size_t)K);
                    tqc_host_sort_row(v.data(), M, K, got.data());
                    bool same = true;
                    for (int k = 0; k < K; k++) same = same && bits(got[(size_t)k]) == bits(v[(size_t)want[(size_t)k]]);
                    CHECK(same, "M %d %s: the host sort's first %d differ from std::stable_sort's", M, kinds[kind], K);
                }
                float nv[EV2G_TQC_MAX_ATOMS];
                int ni[EV2G_TQC_MAX_ATOMS];
                network_sort(v.data(), M, nv, ni);
                bool same = true;
                for (int m = 0; m < M; m++) same = same && ni[m] == want[(size_t)m] && bits(nv[m]) == bits(v[(size_t)want[(size_t)m]]);
                for (int m = M; m < EV2G_TQC_MAX_ATOMS; m++) same = same && ni[m] == m && std::isinf(nv[m]);   // the padding stays behind, in slot order
                CHECK(same, "M %d %s: the network's order differs from std::stable_sort's", M, kinds[kind]);
            }
    CHECK(ev2g_tqc_key_less(0.0f, 1, -0.0f, 2) && !ev2g_tqc_key_less(-0.0f, 2, 0.0f, 1) && ev2g_tqc_key_less(-1.0f, 9, 0.0f, 0), "the key: +0 and -0 by index");
}

// ---- c. the twins ----
static void check_twins() {
    const int B = 37, nc = 3, nq = 7, drop = 1, M = nc * nq, K = nc * (nq - drop);
    std::vector<float> tq((size_t)nc * B * nq), q((size_t)nc * B * nq), lp((size_t)B), r((size_t)B), z((size_t)B * K), dq((size_t)nc * B * nq);
    std::vector<uint8_t> done((size_t)B);
    for (size_t i = 0; i < tq.size(); i++) { tq[i] = rnd(i) * 4.0f; q[i] = rnd(90000 + i) * 4.0f; }
    for (int b = 0; b < B; b++) { lp[(size_t)b] = rnd(5000 + (uint64_t)b) * 6.0f - 4.0f; r[(size_t)b] = rnd(7000 + (uint64_t)b) * 3.0f; done[(size_t)b] = (uint8_t)(hash64(8000 + (uint64_t)b) & 1); }
    const float la = (float)std::log(0.3);
    const double alpha = std::exp((double)la);
    tqc_host_target(tq.data(), lp.data(), r.data(), done.data(), B, nc, nq, drop, 0.99, la, z.data());
    double loss = 0.0;
    int regions[4] = {0, 0, 0, 0};
    std::vector<double> want_dq((size_t)nc * B * nq, 0.0);
    for (int b = 0; b < B; b++) {
        std::vector<float> pool((size_t)M);
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nq; i++) pool[(size_t)(j * nq + i)] = tq[((size_t)j * B + b) * nq + i];
        std::stable_sort(pool.begin(), pool.end());
        for (int k = 0; k < K; k++) {
            const double w = (double)r[(size_t)b] + (done[(size_t)b] ? 0.0 : 0.99) * ((double)pool[(size_t)k] - alpha * (double)lp[(size_t)b]);
            CHECK(bits(z[(size_t)b * K + k]) == bits((float)w), "z[%d, %d]", b, k);
        }
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nq; i++) {
                const size_t at = ((size_t)j * B + b) * nq + i;
                const double tau = (i + 0.5) / nq;
                for (int k = 0; k < K; k++) {
                    const double d = (double)z[(size_t)b * K + k] - (double)q[at], w = std::fabs(tau - (d < 0.0 ? 1.0 : 0.0)), ad = std::fabs(d);
                    loss += w * (ad > 1.0 ? ad - 0.5 : 0.5 * d * d);
                    want_dq[at] -= w * std::fmin(std::fmax(d, -1.0), 1.0);
                    regions[d < -1.0 ? 0 : d < 0.0 ? 1 : d <= 1.0 ? 2 : 3]++;
                }
            }
    }
    const double n_terms = (double)B * nc * nq * K;
    const float got_loss = tqc_host_critic_head(z.data(), q.data(), B, nc, nq, K, dq.data());
    CHECK(std::fabs(got_loss - loss / n_terms) <= 1.2e-7 * (loss / n_terms), "critic loss %g vs %g", got_loss, loss / n_terms);
    double scale = 0.0;
    for (double d : want_dq) scale = std::fmax(scale, std::fabs(d / n_terms));
    for (size_t i = 0; i < dq.size(); i++) CHECK(std::fabs(dq[i] - want_dq[i] / n_terms) <= 1.2e-7 * scale, "dq[%zu] %g vs %g", i, dq[i], want_dq[i] / n_terms);
    for (int g = 0; g < 4; g++) CHECK(regions[g] * 20 >= (int)n_terms, "Huber region %d holds %d of %d deltas", g, regions[g], (int)n_terms);
    // one atom: z is SAC's y
    std::vector<float> y((size_t)B), z1((size_t)B);
    sac_host_y(tq.data(), lp.data(), r.data(), done.data(), B, 1, 0.99, la, y.data());
    std::vector<float> tq1((size_t)B);
    for (int b = 0; b < B; b++) tq1[(size_t)b] = tq[(size_t)b];   // sac_host_y read tq as [1, B]
    tqc_host_target(tq1.data(), lp.data(), r.data(), done.data(), B, 1, 1, 0, 0.99, la, z1.data());
    CHECK(std::memcmp(y.data(), z1.data(), (size_t)B * sizeof(float)) == 0, "one critic of one quantile: z is SAC's y");
    // the actor's head
    float out4[4];
    tqc_host_actor_head(q.data(), lp.data(), B, nc, nq, la, -5.0, 1, out4);
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < B; b++) {
        double m = 0.0;
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nq; i++) m += (double)q[((size_t)j * B + b) * nq + i];
        s1 += alpha * (double)lp[(size_t)b] - m / M; s2 += (double)lp[(size_t)b] - 5.0;
    }
    CHECK(std::fabs(out4[0] - s1 / B) <= 1.2e-7 * std::fabs(s1 / B) + 1e-7 && std::fabs(out4[3] + s2 / B) <= 1.2e-7 * std::fabs(s2 / B) &&
          std::fabs(out4[1] - (double)la * (-s2 / B)) <= 2.4e-7 * std::fabs((double)la * s2 / B) && out4[2] == (float)alpha, "the actor's head");
    tqc_host_actor_head(q.data(), lp.data(), B, nc, nq, la, -5.0, 0, out4);
    CHECK(out4[1] == 0.0f && out4[3] == 0.0f && out4[2] == (float)alpha, "a fixed coefficient");
}

int main() {
    check_plan();
    check_sort();
    check_twins();
    if (fails) { std::printf("tqc_check: %d of %d checks FAILED\n", fails, checks); return 1; }
    std::printf("tqc_check: ok (%d checks)\n", checks);
    return 0;
}
