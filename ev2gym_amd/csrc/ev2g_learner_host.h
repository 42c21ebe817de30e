// ev2g_learner_host.h -- the host-only description of a learner (ev2g_ppo.h): what PPO and A2C differ in, resolved once from a config.
//
// learner_spec(config) is the whole decision: the head of the gradient kernel, the hyper-parameters its launches pass, the optimiser with its
// rate and constants, whether the head reads old_log_prob, and what advantage normalisation does with a single row.  learner_refusal checks a
// config (or the fields a set-rate entry sets) against a table of {field, value, rule}; adam_step / rms_step turn the optimiser's numbers into
// what the apply kernels take; learner_host_head is the host twin of the gradient kernel's head for either kind.  ev2g_host.hip is the device
// stage: it stores one LearnerSpec per learner and launches from it.  Nothing here needs HIP or a handle, so a plain C++17 program can check
// it (tests/host/learner_check.cpp; it defines __host__ and __device__ to nothing for the element functions of ev2g_ppo.h).
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "../../include/ev2g.h"
#include "ev2g_ppo.h"

enum LearnerKind { LEARNER_PPO = 0, LEARNER_A2C = 1, LEARNER_TRPO = 2 };   // which entries drive the learner (ev2g_ppo_* / ev2g_a2c_* / ev2g_trpo_*)
enum LearnerHead { LEARNER_HEAD_PPO = 0, LEARNER_HEAD_A2C = 1 };   // ev2g_ppo_grad_kernel's HEAD (EV2G_HEAD_*: ev2g_host.hip asserts they agree)
enum LearnerOptimiser { LEARNER_ADAM = 0, LEARNER_RMSPROP = 1 };   // ev2g_ppo_apply_kernel / ev2g_a2c_apply_kernel

struct LearnerSpec {
    int kind = LEARNER_PPO, head = LEARNER_HEAD_PPO;
    PpoHyper hyper{};             // what the gradient and reduce launches pass (clip is 0 for a head without a ratio)
    double ent_coef = 0.0;        // the config's float64 value: the host twin subtracts it from d loss / d log_std before the one rounding
    double max_grad_norm = 0.0;
    int optimiser = LEARNER_ADAM;
    double lr = 0.0, beta1 = 0.0, beta2 = 0.0, alpha = 0.0, eps = 0.0;   // Adam: lr, beta1, beta2, eps; RMSprop: lr, alpha, eps
    bool reads_old_lp = true;     // the head reads old_log_prob (else the launch passes null)
    bool one_row_norm_refused = false;   // normalize_advantage with B == 1: refused (A2C: SB3 would produce NaN), else skipped silently (PPO)
    const char *grad_entry = "ev2g_ppo_grad";   // the entry the "no gradient to apply" refusal points at
};

inline LearnerSpec learner_spec(const ev2g_ppo_config &c) {
    LearnerSpec s;
    s.hyper = {(float)c.clip_range, (float)c.vf_coef, (float)c.ent_coef, c.normalize_advantage ? 1 : 0};
    s.ent_coef = c.ent_coef; s.max_grad_norm = c.max_grad_norm;
    s.lr = c.lr; s.beta1 = c.beta1; s.beta2 = c.beta2; s.eps = c.adam_eps;
    return s;
}

inline LearnerSpec learner_spec(const ev2g_a2c_config &c) {
    LearnerSpec s;
    s.kind = LEARNER_A2C; s.head = LEARNER_HEAD_A2C;
    s.hyper = {0.0f, (float)c.vf_coef, (float)c.ent_coef, c.normalize_advantage ? 1 : 0};
    s.ent_coef = c.ent_coef; s.max_grad_norm = c.max_grad_norm;
    s.lr = c.lr;
    if (c.use_rms_prop) { s.optimiser = LEARNER_RMSPROP; s.alpha = c.alpha; s.eps = c.rms_eps; }
    else { s.beta1 = 0.9; s.beta2 = 0.999; s.eps = 1e-5; }   // what SB3's policy builds when RMSprop is switched off: torch.optim.Adam(eps = 1e-5)
    s.reads_old_lp = false; s.one_row_norm_refused = true;
    s.grad_entry = "ev2g_a2c_grad";
    return s;
}

// ---- config checks: one checker over {field name, value, rule}, the fields in the order their refusals have always been reported in ----
enum LearnerRule { LEARNER_GE0 = 0, LEARNER_GT0, LEARNER_UNIT, LEARNER_UNIT_CLOSED, LEARNER_GE1 };   // (the last two: the TD3 learner's tau / gamma and policy_delay)
struct LearnerField { const char *name; double value; int rule; };

// the fields the set-rate entries set (ev2g_ppo_set_rates, ev2g_a2c_set_rate); a config's list starts with them
inline std::vector<LearnerField> ppo_rate_fields(double lr, double clip_range) { return {{"lr", lr, LEARNER_GE0}, {"clip_range", clip_range, LEARNER_GT0}}; }
inline std::vector<LearnerField> a2c_rate_fields(double lr) { return {{"lr", lr, LEARNER_GE0}}; }

inline std::vector<LearnerField> learner_fields(const ev2g_ppo_config &c) {
    std::vector<LearnerField> f = ppo_rate_fields(c.lr, c.clip_range);
    f.insert(f.end(), {{"beta1", c.beta1, LEARNER_UNIT}, {"beta2", c.beta2, LEARNER_UNIT}, {"adam_eps", c.adam_eps, LEARNER_GT0}, {"vf_coef", c.vf_coef, LEARNER_GE0},
                       {"ent_coef", c.ent_coef, LEARNER_GE0}, {"max_grad_norm", c.max_grad_norm, LEARNER_GT0}});
    return f;
}
inline std::vector<LearnerField> learner_fields(const ev2g_a2c_config &c) {
    std::vector<LearnerField> f = a2c_rate_fields(c.lr);
    f.insert(f.end(), {{"alpha", c.alpha, LEARNER_UNIT}, {"rms_eps", c.rms_eps, LEARNER_GT0}, {"vf_coef", c.vf_coef, LEARNER_GE0}, {"ent_coef", c.ent_coef, LEARNER_GE0},
                       {"max_grad_norm", c.max_grad_norm, LEARNER_GT0}});
    return f;
}

// the EV2G_ERR_ARG message of the first field that breaks its rule ("<who>: <field> must be <range>"), or empty
inline std::string learner_refusal(const char *who, const std::vector<LearnerField> &fields) {
    static const char *const range[] = {"finite and >= 0", "finite and > 0", "in [0, 1)", "in [0, 1]", "finite and >= 1"};
    for (const LearnerField &f : fields) {
        const double v = f.value;
        const bool ok = std::isfinite(v) && (f.rule == LEARNER_GE0 ? v >= 0.0 : f.rule == LEARNER_GT0 ? v > 0.0 : f.rule == LEARNER_UNIT ? v >= 0.0 && v < 1.0
                                              : f.rule == LEARNER_UNIT_CLOSED ? v >= 0.0 && v <= 1.0 : v >= 1.0);
        if (!ok) return std::string(who) + ": " + f.name + " must be " + range[f.rule];
    }
    return std::string();
}

// ---- what the apply kernels take: float64 intermediates, each member rounded to float once ----
inline AdamStep adam_step(double lr, double beta1, double beta2, double eps, long long t) {
    const double bc1 = 1.0 - std::pow(beta1, (double)t), bc2 = 1.0 - std::pow(beta2, (double)t);
    return {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1), (float)std::sqrt(bc2), (float)eps};
}

inline RmsStep rms_step(double lr, double alpha, double eps) { return {(float)alpha, (float)(1.0 - alpha), (float)lr, (float)eps}; }

// ---- the host twin of the gradient kernel's head (ev2g_host_ppo_head, ev2g_host_a2c_head): d loss / d mean [B, P], d loss / d value [B],
// d loss / d log_std [P] (entropy term included) and the six statistics; old_log_prob is read only if the head reads it.  B >= 1, P >= 1, and
// not one normalised row where the spec refuses it: the caller's checks.  Every sum runs rows ascending, a row's log-probability over eight
// partial sums joined as the device's butterfly joins them.
inline void learner_host_head(const LearnerSpec &spec, const float *mean, const float *value, const float *actions, const float *log_std,
                              const float *old_log_prob, const float *advantages, const float *returns, int B, int P, float *d_mean, float *d_value,
                              float *d_log_std, float *stats) {
    const PpoHyper &hp = spec.hyper;
    const bool norm = hp.normalize && B > 1;
    double a_mean = 0.0, a_scale = 1.0;
    if (norm) {
        double s = 0.0;
        for (int i = 0; i < B; i++) s += (double)advantages[i];
        a_mean = s / B;
        s = 0.0;
        for (int i = 0; i < B; i++) { const double d = (double)advantages[i] - a_mean; s += d * d; }
        a_scale = 1.0 / (std::sqrt(s / (double)(B - 1)) + 1e-8);
    }
    std::vector<double> iv((size_t)P), dls((size_t)P, 0.0);
    for (int p = 0; p < P; p++) iv[(size_t)p] = std::exp(-2.0 * (double)log_std[p]);
    const double inv_b = 1.0 / (double)B;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < B; i++) {
        const float *mu = mean + (size_t)i * P, *a = actions + (size_t)i * P;
        double q[8];
        for (int j = 0; j < 8; j++) q[j] = ev2g_ppo_lp_part(mu, a, log_std, iv.data(), P, j, 8);
        const float A = norm ? (float)(((double)advantages[i] - a_mean) * a_scale) : advantages[i];
        const PpoRow o = spec.head == LEARNER_HEAD_PPO ? ev2g_ppo_head_row(ev2g_ppo_join8(q), old_log_prob[i], A, returns[i], value[i], hp.clip, hp.vf_coef, inv_b)
                                                       : ev2g_a2c_head_row(ev2g_ppo_join8(q), A, returns[i], value[i], hp.vf_coef, inv_b);
        d_value[i] = o.g_v;
        sum[0] += o.pol; sum[1] += o.vsq; sum[2] += o.kl; sum[3] += o.clipped;
        for (int p = 0; p < P; p++) {
            float dl;
            ev2g_ppo_head_port(a[p], mu[p], iv[(size_t)p], o.g_lp, d_mean + (size_t)i * P + p, &dl);
            dls[(size_t)p] += (double)dl;
        }
    }
    for (int p = 0; p < P; p++) d_log_std[p] = (float)(dls[(size_t)p] - spec.ent_coef);
    ev2g_ppo_stats(sum, log_std, P, inv_b, hp.vf_coef, hp.ent_coef, stats);
}
