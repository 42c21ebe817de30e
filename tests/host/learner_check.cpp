// The learners' host-only description (csrc/ev2g_learner_host.h), without HIP:
//   * learner_spec of SB3's default PPO config and of SB3's default A2C config (use_rms_prop 1 and 0) has the head, the optimiser, its constants
//     and the hyper-parameters written out here by hand;
//   * learner_refusal refuses every out-of-range, NaN and infinite value of every config field with the message the ABI has always given (the
//     strings below are literal copies), names the earlier of two bad fields, and the set-rate lists refuse the same values of their fields;
//   * adam_step at t = 1, 2 and 1000 and rms_step equal expressions written independently here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#define __host__
#define __device__
#include "../../ev2gym_amd/csrc/ev2g_learner_host.h"

static int fails = 0, checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();
static const ev2g_ppo_config PPO_DEFAULT = {3e-4, 0.9, 0.999, 1e-5, 0.2, 0.5, 0.0, 0.5, 1};
static const ev2g_a2c_config A2C_DEFAULT = {7e-4, 0.99, 1e-5, 0.5, 0.0, 0.5, 0, 1};

static void check_default_specs() {
    const LearnerSpec p = learner_spec(PPO_DEFAULT);
    CHECK(p.kind == LEARNER_PPO && p.head == LEARNER_HEAD_PPO && p.head == 0, "PPO: kind %d head %d", p.kind, p.head);
    CHECK(p.hyper.clip == 0.2f && p.hyper.vf_coef == 0.5f && p.hyper.ent_coef == 0.0f && p.hyper.normalize == 1, "PPO: hyper-parameters");
    CHECK(p.ent_coef == 0.0 && p.max_grad_norm == 0.5, "PPO: ent_coef, max_grad_norm");
    CHECK(p.optimiser == LEARNER_ADAM && p.lr == 3e-4 && p.beta1 == 0.9 && p.beta2 == 0.999 && p.eps == 1e-5, "PPO: Adam(3e-4, 0.9, 0.999, 1e-5)");
    CHECK(p.reads_old_lp && !p.one_row_norm_refused && std::strcmp(p.grad_entry, "ev2g_ppo_grad") == 0, "PPO: old_log_prob, one row, the grad entry");

    const LearnerSpec a = learner_spec(A2C_DEFAULT);
    CHECK(a.kind == LEARNER_A2C && a.head == LEARNER_HEAD_A2C && a.head == 1, "A2C: kind %d head %d", a.kind, a.head);
    CHECK(a.hyper.clip == 0.0f && a.hyper.vf_coef == 0.5f && a.hyper.ent_coef == 0.0f && a.hyper.normalize == 0, "A2C: hyper-parameters");
    CHECK(a.ent_coef == 0.0 && a.max_grad_norm == 0.5, "A2C: ent_coef, max_grad_norm");
    CHECK(a.optimiser == LEARNER_RMSPROP && a.lr == 7e-4 && a.alpha == 0.99 && a.eps == 1e-5, "A2C: RMSprop(7e-4, 0.99, 1e-5)");
    CHECK(!a.reads_old_lp && a.one_row_norm_refused && std::strcmp(a.grad_entry, "ev2g_a2c_grad") == 0, "A2C: old_log_prob, one row, the grad entry");

    ev2g_a2c_config c = A2C_DEFAULT;
    c.use_rms_prop = 0; c.alpha = 0.5; c.rms_eps = 1e-3;   // (RMSprop's numbers are not Adam's)
    const LearnerSpec b = learner_spec(c);
    CHECK(b.kind == LEARNER_A2C && b.head == LEARNER_HEAD_A2C && !b.reads_old_lp && b.one_row_norm_refused, "A2C with Adam: still A2C's head");
    CHECK(b.optimiser == LEARNER_ADAM && b.lr == 7e-4 && b.beta1 == 0.9 && b.beta2 == 0.999 && b.eps == 1e-5, "A2C with Adam: Adam(7e-4, 0.9, 0.999, 1e-5)");

    ev2g_ppo_config e = PPO_DEFAULT;
    e.ent_coef = 0.01; e.normalize_advantage = 0; e.clip_range = 0.1;
    const LearnerSpec q = learner_spec(e);
    CHECK(q.ent_coef == 0.01 && q.hyper.ent_coef == 0.01f && q.hyper.normalize == 0 && q.hyper.clip == 0.1f, "PPO: the config's numbers reach the spec");
}

// one field of a config: its name, where it lives, the values it refuses besides NaN and the infinities, a value it accepts, the message's tail
template <class CONFIG>
struct Field { const char *name; double CONFIG::*at; double bad[2]; int n_bad; double good; const char *tail; };

static const Field<ev2g_ppo_config> PPO_FIELDS[] = {
    {"lr", &ev2g_ppo_config::lr, {-1e-9, 0}, 1, 0.0, ": lr must be finite and >= 0"},
    {"clip_range", &ev2g_ppo_config::clip_range, {0.0, -0.2}, 2, 1e-9, ": clip_range must be finite and > 0"},
    {"beta1", &ev2g_ppo_config::beta1, {-0.1, 1.0}, 2, 0.0, ": beta1 must be in [0, 1)"},
    {"beta2", &ev2g_ppo_config::beta2, {-0.1, 1.0}, 2, 0.0, ": beta2 must be in [0, 1)"},
    {"adam_eps", &ev2g_ppo_config::adam_eps, {0.0, -1e-5}, 2, 1e-12, ": adam_eps must be finite and > 0"},
    {"vf_coef", &ev2g_ppo_config::vf_coef, {-1.0, 0}, 1, 0.0, ": vf_coef must be finite and >= 0"},
    {"ent_coef", &ev2g_ppo_config::ent_coef, {-0.01, 0}, 1, 0.0, ": ent_coef must be finite and >= 0"},
    {"max_grad_norm", &ev2g_ppo_config::max_grad_norm, {0.0, -0.5}, 2, 1e-9, ": max_grad_norm must be finite and > 0"},
};
static const Field<ev2g_a2c_config> A2C_FIELDS[] = {
    {"lr", &ev2g_a2c_config::lr, {-1e-9, 0}, 1, 0.0, ": lr must be finite and >= 0"},
    {"alpha", &ev2g_a2c_config::alpha, {-0.1, 1.0}, 2, 0.0, ": alpha must be in [0, 1)"},
    {"rms_eps", &ev2g_a2c_config::rms_eps, {0.0, -1e-5}, 2, 1e-12, ": rms_eps must be finite and > 0"},
    {"vf_coef", &ev2g_a2c_config::vf_coef, {-1.0, 0}, 1, 0.0, ": vf_coef must be finite and >= 0"},
    {"ent_coef", &ev2g_a2c_config::ent_coef, {-0.01, 0}, 1, 0.0, ": ent_coef must be finite and >= 0"},
    {"max_grad_norm", &ev2g_a2c_config::max_grad_norm, {0.0, -0.5}, 2, 1e-9, ": max_grad_norm must be finite and > 0"},
};

template <class CONFIG, size_t N>
static void check_refusals(const char *who, const CONFIG &def, const Field<CONFIG> (&fields)[N]) {
    CHECK(learner_refusal(who, learner_fields(def)).empty(), "%s refuses the default config: %s", who, learner_refusal(who, learner_fields(def)).c_str());
    for (size_t i = 0; i < N; i++) {
        const Field<CONFIG> &f = fields[i];
        const std::string want = std::string(who) + f.tail;
        std::vector<double> bad(f.bad, f.bad + f.n_bad);
        bad.insert(bad.end(), {NaN, Inf, -Inf});
        for (double v : bad) {
            CONFIG c = def;
            c.*(f.at) = v;
            const std::string got = learner_refusal(who, learner_fields(c));
            CHECK(got == want, "%s = %g: '%s', expected '%s'", f.name, v, got.c_str(), want.c_str());
            for (size_t j = i + 1; j < N; j++) {   // a later bad field as well: the earlier one is named
                CONFIG c2 = c;
                c2.*(fields[j].at) = NaN;
                CHECK(learner_refusal(who, learner_fields(c2)) == want, "%s = %g and %s = nan: the earlier field is not the one named", f.name, v, fields[j].name);
            }
        }
        CONFIG c = def;
        c.*(f.at) = f.good;
        CHECK(learner_refusal(who, learner_fields(c)).empty(), "%s = %g is refused", f.name, f.good);
    }
}

static void check_rate_fields() {
    CHECK(learner_refusal("ev2g_ppo_set_rates", ppo_rate_fields(0.0, 0.3)).empty() && learner_refusal("ev2g_a2c_set_rate", a2c_rate_fields(0.0)).empty(), "rates in range");
    for (double v : {-1.0, NaN, Inf, -Inf}) {
        CHECK(learner_refusal("ev2g_ppo_set_rates", ppo_rate_fields(v, 0.2)) == "ev2g_ppo_set_rates: lr must be finite and >= 0", "set_rates lr %g", v);
        CHECK(learner_refusal("ev2g_ppo_set_rates", ppo_rate_fields(v, NaN)) == "ev2g_ppo_set_rates: lr must be finite and >= 0", "set_rates lr %g before clip_range", v);
        CHECK(learner_refusal("ev2g_a2c_set_rate", a2c_rate_fields(v)) == "ev2g_a2c_set_rate: lr must be finite and >= 0", "set_rate lr %g", v);
    }
    for (double v : {0.0, -0.2, NaN, Inf, -Inf})
        CHECK(learner_refusal("ev2g_ppo_set_rates", ppo_rate_fields(3e-4, v)) == "ev2g_ppo_set_rates: clip_range must be finite and > 0", "set_rates clip_range %g", v);
}

static void check_steps() {
    const double lr = 3e-4, b1 = 0.9, b2 = 0.999, eps = 1e-5;
    for (long long t : {1LL, 2LL, 1000LL}) {
        const AdamStep a = adam_step(lr, b1, b2, eps, t);
        double p1 = 1.0, p2 = 1.0;   // beta^t by repeated multiplication: exact enough to agree with pow after the rounding to float
        for (long long k = 0; k < t; k++) { p1 *= b1; p2 *= b2; }
        const float step_size = (float)(lr / (1.0 - std::pow(b1, (double)t))), bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)t));
        CHECK(a.omb1 == (float)(1.0 - 0.9) && a.beta2 == 0.999f && a.omb2 == (float)(1.0 - 0.999) && a.eps == 1e-5f, "adam_step t %lld: the constants", t);
        CHECK(a.step_size == step_size && a.bc2_sqrt == bc2_sqrt, "adam_step t %lld: step_size %.9g bc2_sqrt %.9g", t, a.step_size, a.bc2_sqrt);
        CHECK(std::fabs((double)a.step_size - lr / (1.0 - p1)) <= 1e-7 * lr / (1.0 - p1) && std::fabs((double)a.bc2_sqrt - std::sqrt(1.0 - p2)) <= 1e-7,
              "adam_step t %lld against beta^t by multiplication", t);
    }
    const AdamStep one = adam_step(lr, b1, b2, eps, 1);
    CHECK(one.step_size == (float)(3e-4 / (1.0 - 0.9)) && one.bc2_sqrt == (float)std::sqrt(1.0 - 0.999), "adam_step t 1 by hand");
    const AdamStep two = adam_step(lr, b1, b2, eps, 2);
    CHECK(two.step_size == (float)(3e-4 / (1.0 - 0.9 * 0.9)) && two.bc2_sqrt == (float)std::sqrt(1.0 - 0.999 * 0.999), "adam_step t 2 by hand");
    CHECK(one.omb1 != 1.0f - 0.9f || one.omb2 != 1.0f - 0.999f, "1 - beta is rounded from float64, not computed in float");
    const RmsStep r = rms_step(7e-4, 0.99, 1e-5);
    CHECK(r.alpha == 0.99f && r.oma == (float)(1.0 - 0.99) && r.lr == 7e-4f && r.eps == 1e-5f, "rms_step");
}

// learner_host_head runs both heads over the same rows: A2C's ratio statistics are exact zeros, PPO's one normalised row is the row itself
static void check_host_head() {
    const int B = 3, P = 5;
    float mean[B * P], act[B * P], value[B] = {0.25f, -0.5f, 1.0f}, ls[P], old_lp[B] = {-4.0f, -5.0f, -6.0f}, adv[B] = {1.0f, -2.0f, 0.5f}, ret[B] = {0.5f, 0.0f, 1.5f};
    for (int i = 0; i < B * P; i++) { mean[i] = 0.01f * (float)i; act[i] = 0.3f - 0.02f * (float)i; }
    for (int p = 0; p < P; p++) ls[p] = -0.5f + 0.1f * (float)p;
    ev2g_ppo_config pc = PPO_DEFAULT;
    ev2g_a2c_config ac = A2C_DEFAULT;
    pc.ent_coef = ac.ent_coef = 0.01;
    float dm[2][B * P], dv[2][B], dl[2][P], st[2][6];
    learner_host_head(learner_spec(pc), mean, value, act, ls, old_lp, adv, ret, B, P, dm[0], dv[0], dl[0], st[0]);
    learner_host_head(learner_spec(ac), mean, value, act, ls, nullptr, adv, ret, B, P, dm[1], dv[1], dl[1], st[1]);
    CHECK(st[1][4] == 0.0f && st[1][5] == 0.0f && st[0][4] != 0.0f, "A2C's ratio statistics are exact zeros, PPO's are not");
    CHECK(std::memcmp(dv[0], dv[1], sizeof dv[0]) == 0 && st[0][1] == st[1][1] && st[0][2] == st[1][2], "the value and entropy terms do not depend on the head");
    for (int k = 0; k < 2; k++)
        for (int p = 0; p < P; p++) CHECK(std::isfinite(dl[k][p]) && std::isfinite(dm[k][p]), "head %d port %d", k, p);
    pc.normalize_advantage = 0;
    learner_host_head(learner_spec(pc), mean, value, act, ls, old_lp, adv, ret, 1, P, dm[1], dv[1], dl[1], st[1]);
    pc.normalize_advantage = 1;
    learner_host_head(learner_spec(pc), mean, value, act, ls, old_lp, adv, ret, 1, P, dm[0], dv[0], dl[0], st[0]);
    CHECK(std::memcmp(dl[0], dl[1], sizeof dl[0]) == 0 && std::memcmp(st[0], st[1], sizeof st[0]) == 0, "PPO skips the normalisation of one row");
}

int main() {
    check_default_specs();
    check_host_head();
    check_refusals("ev2g_ppo_create", PPO_DEFAULT, PPO_FIELDS);
    check_refusals("ev2g_a2c_create", A2C_DEFAULT, A2C_FIELDS);
    check_rate_fields();
    check_steps();
    if (fails) return 1;
    std::printf("learner_check: ok (%d checks)\n", checks);
    return 0;
}
