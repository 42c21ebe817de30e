// The TRPO learner's host-only half (csrc/ev2g_trpo_host.h), without HIP:
//   * plan_trpo accepts every network plan_ppo accepts, refuses what it refuses with its message, never takes more LDS than PPO's plan, its
//     LDS blocks do not overlap and end at `bytes`, and the flat actor order is log_std | pi_W1 | pi_b1 | pi_W2 | pi_b2 | action_W | action_b;
//   * trpo_map places every actor element exactly once, with the image widths ac_params gives;
//   * learner_fields(ev2g_trpo_config) refuses every out-of-range value by the field's name, and accepts sb3_contrib's defaults;
//   * trpo_host_cg_step solves a small SPD system as a dense solve does and takes the 1e-10 exit; trpo_host_rows equals expressions written
//     independently here.
// A plain program with its own main: it is also the one to build with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#define __host__
#define __device__
#include "../../ev2gym_amd/csrc/ev2g_trpo_host.h"

static int fails = 0, checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

static const ev2g_trpo_config DEFAULT = {1e-3, 0.01, 0.1, 0.8, 15, 10, 1};

static void check_plans() {
    const int nets[][6] = {{63, 64, 64, 64, 64, 20}, {162, 64, 64, 64, 64, 50}, {63, 128, 128, 128, 128, 20}, {162, 256, 32, 32, 96, 50}, {192, 96, 160, 160, 32, 64},
                           {5, 8, 8, 8, 8, 1}, {33, 64, 64, 64, 64, 33}, {1, 1, 1, 1, 1, 1}, {63, 33, 17, 40, 64, 20}, {192, 64, 64, 64, 64, 64}};
    for (const auto &n : nets) {
        const PpoPlan pp = plan_ppo(n[0], n[1], n[2], n[3], n[4], n[5]);
        const TrpoPlan tp = plan_trpo(n[0], n[1], n[2], n[3], n[4], n[5]);
        CHECK(!pp.err && !tp.err, "net %d: refused", n[0]);
        CHECK(tp.lds.bytes <= pp.lds.bytes && tp.lds.bytes <= EV2G_PPO_LDS_LIMIT, "net %d: LDS %zu > PPO's %zu", n[0], tp.lds.bytes, pp.lds.bytes);
        const TrpoLds &l = tp.lds;
        const int R = EV2G_PPO_ROWS, n3 = tp.ppo.ac.n3;
        const int off[] = {l.oIV, l.oKC, l.oKQ, l.oX, l.oH1, l.oH2, l.oT1, l.oT2, l.oMU, l.oACT, l.oROW};
        const int len[] = {2 * n3, 2 * n3, 2 * n3, R * l.sX, R * l.sA, R * l.sB, R * l.sA, R * l.sB, R * l.sMU, R * l.sMU, 3 * R};
        int o = 0;
        for (int i = 0; i < 11; i++) { CHECK(off[i] == o, "net %d: block %d at %d, not %d", n[0], i, off[i], o); o += len[i]; }
        CHECK((size_t)o * sizeof(float) == l.bytes && l.oX % 2 == 0, "net %d: bytes", n[0]);
        CHECK(l.sA >= tp.ppo.ac.n1 + 4 && l.sA >= tp.ppo.ac.m1 + 4 && l.sB >= tp.ppo.ac.n2 + 4 && l.sB >= tp.ppo.ac.m2 + 4, "net %d: strides", n[0]);
        const int want = n[5] + n[1] * n[0] + n[1] + n[2] * n[1] + n[2] + n[5] * n[2] + n[5];
        CHECK(tp.n_actor == want && tp.off[EV2G_TRPO_ACTOR_ARRAYS] == want, "net %d: n_actor %d, not %d", n[0], tp.n_actor, want);
        const int order[] = {12, 0, 1, 2, 3, 8, 9};
        for (int k = 0; k < EV2G_TRPO_ACTOR_ARRAYS; k++) CHECK(tp.arr[k] == order[k], "net %d: actor array %d", n[0], k);
        float *dimg[EV2G_TRPO_ACTOR_ARRAYS] = {};
        const TrpoMap m = trpo_map(tp, dimg);
        const auto tab = ac_params(tp.ppo.ac);
        std::vector<int> seen((size_t)tp.ppo.n_params, 0);
        for (int k = 0; k < EV2G_TRPO_ACTOR_ARRAYS; k++) {
            CHECK(m.img_k[k] == tab[(size_t)order[k]].img_k && m.cols[k] == tp.ppo.cols[order[k]], "net %d: map of array %d", n[0], k);
            for (int i = m.off[k]; i < m.off[k + 1]; i++) seen[(size_t)(tp.ppo.off[order[k]] + i - m.off[k])]++;
        }
        int once = 0;
        for (int v : seen) once += v == 1;
        CHECK(once == want, "net %d: %d master elements addressed once, not %d", n[0], once, want);
    }
    const int bad[][6] = {{193, 64, 64, 64, 64, 50}, {162, 64, 64, 64, 64, 65}, {162, 64, 0, 64, 64, 50}, {192, 128, 128, 128, 128, 64}};
    for (const auto &n : bad) {
        const PpoPlan pp = plan_ppo(n[0], n[1], n[2], n[3], n[4], n[5]);
        const TrpoPlan tp = plan_trpo(n[0], n[1], n[2], n[3], n[4], n[5]);
        CHECK(pp.err == EV2G_ERR_ARG && tp.err == EV2G_ERR_ARG && tp.refusal == pp.refusal, "bad net %d: '%s'", n[0], tp.refusal.c_str());
    }
}

static void check_fields() {
    const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();
    CHECK(learner_refusal("t", learner_fields(DEFAULT)).empty(), "the defaults are refused");
    const TrpoSpec s = trpo_spec(DEFAULT);
    CHECK(s.lr == 1e-3 && s.target_kl == 0.01 && s.cg_damping == 0.1 && s.shrink == 0.8 && s.cg_max_steps == 15 && s.ls_max_iter == 10 && s.normalize == 1, "spec");
    const LearnerSpec l = learner_spec(DEFAULT);
    CHECK(l.kind == LEARNER_TRPO && l.optimiser == LEARNER_ADAM && l.beta1 == 0.9 && l.beta2 == 0.999 && l.eps == 1e-5 && l.lr == 1e-3, "learner spec");
    struct { const char *name; double ev2g_trpo_config::*f; double bad[4]; } dbl[] = {
        {"lr", &ev2g_trpo_config::lr, {-1e-9, NaN, Inf, -Inf}}, {"target_kl", &ev2g_trpo_config::target_kl, {0.0, -1.0, NaN, Inf}},
        {"cg_damping", &ev2g_trpo_config::cg_damping, {-0.1, NaN, Inf, -Inf}},
        {"line_search_shrinking_factor", &ev2g_trpo_config::line_search_shrinking_factor, {0.0, 1.0, NaN, 1.5}}};
    for (const auto &d : dbl)
        for (double v : d.bad) {
            ev2g_trpo_config c = DEFAULT;
            c.*(d.f) = v;
            const std::string r = learner_refusal("t", learner_fields(c));
            CHECK(r.rfind(std::string("t: ") + d.name + " must be", 0) == 0, "%s = %g: '%s'", d.name, v, r.c_str());
        }
    for (int v : {0, -1}) {
        ev2g_trpo_config c = DEFAULT;
        c.cg_max_steps = v;
        CHECK(learner_refusal("t", learner_fields(c)) == "t: cg_max_steps must be finite and >= 1", "cg_max_steps %d", v);
        c = DEFAULT;
        c.line_search_max_iter = v;
        CHECK(learner_refusal("t", learner_fields(c)) == "t: line_search_max_iter must be finite and >= 1", "line_search_max_iter %d", v);
    }
    ev2g_trpo_config two = DEFAULT;
    two.target_kl = 0.0; two.cg_max_steps = 0;
    CHECK(learner_refusal("t", learner_fields(two)).find("target_kl") != std::string::npos, "the earlier of two bad fields is named");
}

static void check_cg() {
    // H = tridiag(-1, 2.5, -1), n = 12: conjugate gradient against Gaussian elimination
    const int n = 12;
    std::vector<double> g((size_t)n), x((size_t)n, 0.0), r, p, hp((size_t)n);
    for (int i = 0; i < n; i++) g[(size_t)i] = 1.0 + 0.25 * i;
    auto mul = [&](const std::vector<double> &v, std::vector<double> &o) {
        for (int i = 0; i < n; i++) o[(size_t)i] = 2.5 * v[(size_t)i] - (i ? v[(size_t)i - 1] : 0.0) - (i + 1 < n ? v[(size_t)i + 1] : 0.0);
    };
    r = g; p = g;
    double rho = 0.0;
    for (double v : g) rho += v * v;
    int iters = 0, done = 0;
    while (!done && iters < 50) { mul(p, hp); done = trpo_host_cg_step(x.data(), r.data(), p.data(), hp.data(), n, &rho, 0); iters++; }
    CHECK(done && iters <= n && rho < EV2G_TRPO_RHO_MIN, "the solve ends by the 1e-10 exit within n iterations (%d, rho %g)", iters, rho);
    mul(x, hp);
    double err = 0.0;
    for (int i = 0; i < n; i++) err = std::fmax(err, std::fabs(hp[(size_t)i] - g[(size_t)i]));
    CHECK(err < 1e-4, "H x = g to %g", err);
    // `last`: x moves, r and p do not
    std::vector<double> x2((size_t)n, 0.0), r2 = g, p2 = g;
    double rho2 = 0.0;
    for (double v : g) rho2 += v * v;
    const double rho_in = rho2;
    mul(p2, hp);
    CHECK(trpo_host_cg_step(x2.data(), r2.data(), p2.data(), hp.data(), n, &rho2, 1) == 1 && rho2 == rho_in && r2 == g && p2 == g && x2[0] != 0.0, "the last iteration");
}

static void check_rows() {
    const int B = 5, P = 11;   // (P is no multiple of the eight lanes)
    std::vector<float> mu((size_t)B * P), mu0((size_t)B * P), a((size_t)B * P), ls((size_t)P), ls0((size_t)P), old((size_t)B), adv((size_t)B);
    unsigned s = 12345u;
    auto rnd = [&s]() { s = s * 1664525u + 1013904223u; return (float)((s >> 8) & 0xffff) / 65536.0f - 0.5f; };
    for (auto *v : {&mu, &mu0, &a}) for (float &f : *v) f = rnd();
    for (int p = 0; p < P; p++) { ls[(size_t)p] = 0.5f * rnd() - 0.3f; ls0[(size_t)p] = ls[(size_t)p] + 0.05f * rnd(); }
    for (int i = 0; i < B; i++) { old[(size_t)i] = -12.0f + rnd(); adv[(size_t)i] = 2.0f * rnd(); }
    for (int normalize = 0; normalize < 2; normalize++) {
        std::vector<double> j((size_t)B), kl((size_t)B);
        trpo_host_rows(mu.data(), mu0.data(), a.data(), ls.data(), ls0.data(), old.data(), adv.data(), B, P, normalize, j.data(), kl.data());
        double mean = 0.0, var = 0.0;
        for (float v : adv) mean += v;
        mean /= B;
        for (float v : adv) var += (v - mean) * (v - mean);
        const double scale = 1.0 / (std::sqrt(var / (B - 1)) + 1e-8);
        for (int i = 0; i < B; i++) {
            double lp = 0.0, k = 0.0;
            for (int p = 0; p < P; p++) {
                const double l = ls[(size_t)p], l0 = ls0[(size_t)p], d = (double)a[(size_t)i * P + p] - mu[(size_t)i * P + p], e = (double)mu[(size_t)i * P + p] - mu0[(size_t)i * P + p];
                lp += -d * d / (2.0 * std::exp(2.0 * l)) - l - 0.9189385332046727;
                k += l0 - l + (std::exp(2.0 * l) + e * e) / (2.0 * std::exp(2.0 * l0)) - 0.5;
            }
            const double A = normalize ? (double)(float)((adv[(size_t)i] - mean) * scale) : adv[(size_t)i];
            const double want = A * std::exp(lp - old[(size_t)i]);
            CHECK(std::fabs(j[(size_t)i] - want) <= 1e-12 * std::fabs(want) && std::fabs(kl[(size_t)i] - k) <= 1e-12 * std::fabs(k), "row %d normalize %d: %g %g, %g %g", i,
                  normalize, j[(size_t)i], want, kl[(size_t)i], k);
        }
    }
}

int main() {
    check_plans();
    check_fields();
    check_cg();
    check_rows();
    std::printf("trpo_check: %s (%d checks, %d failed)\n", fails ? "FAILED" : "ok", checks, fails);
    return fails ? 1 : 0;
}
