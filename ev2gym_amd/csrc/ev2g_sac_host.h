// ev2g_sac_host.h -- the host-only half of the SAC learner (ev2g_sac.h): which networks it accepts, where every parameter array and every
// workspace block sits, the padded widths of the collection actor's images, the config's checks, and the host twins of the element functions.
//
// plan_sac(d_in, h1, h2, d_out, n_critics) refuses with one message per field, as plan_td3 does, and lays out
//   * the flat parameter buffer (masters, Adam's m and v, the gradient): the actor's W1 | b1 | W2 | b2 | Wmu | bmu | Wls | bls in SB3's [out, in]
//     layout, then the six arrays of critic 0, then critic 1 -- SB3's parameter order (actor.latent_pi.{0,2}, actor.mu, actor.log_std,
//     critic.qf{0,1}.{0,2,4}); the targets are the critics' blocks alone, in the same order;
//   * the workspace of one batch of EV2G_TD3_MAX_BATCH rows (offsets in floats).
// The limits are the collection kernel's: D <= 192, hidden widths <= 256, P <= 64.  Nothing here needs HIP or a handle:
// tests/host/sac_check.cpp enumerates it.
#pragma once
#include <string>
#include <vector>

#include "../../include/ev2g.h"
#include "ev2g_learner_host.h"
#include "ev2g_policy_host.h"
#include "ev2g_td3_host.h"
#include "ev2g_sac.h"

#define EV2G_SAC_MAX_IN 192
#define EV2G_SAC_MAX_HIDDEN 256
#define EV2G_SAC_MAX_OUT 64
#define EV2G_SAC_ACTOR_ARRAYS 8

struct SacPlan {
    int err = EV2G_OK;
    std::string refusal;
    int d_in = 0, h1 = 0, h2 = 0, d_out = 0, nc = 0, da = 0;   // da = d_in + d_out: a critic's input width
    int aoff[EV2G_SAC_ACTOR_ARRAYS + 1] = {}, coff[7] = {};      // the arrays' starts inside the actor's / one critic's block (last: the block's size)
    int n_actor = 0, n_critic = 0, n_params = 0, head_block = 0; // head_block = d_out h2 + d_out: the z stride from (Wmu | bmu) to (Wls | bls)
    int k1 = 0, n1 = 0, n2 = 0, n3 = 0;                          // the collection actor's padded widths (SacDev's)
    // workspace (floats): critic input (s, a~) | (s', a') or (s, a_pi) | the actor's h1, h2 | mu, raw log_std [2][B, P] | eps, a [B, P] | log pi of
    // the actor half, of the critic half [B] | per critic h1, h2 | q, tq [nc, B] | y [B] | dq [nc, B] | per critic deltas d2, d1 | the critics'
    // input deltas [nc][B, P] | d_mu, d_log_std [2][B, P] | the heads' backward-data products [2][B, h2] | the actor's deltas e2, e1
    long long w_xa = 0, w_xb = 0, w_ah1 = 0, w_ah2 = 0, w_head = 0, w_eps = 0, w_a = 0, w_lp = 0, w_lp2 = 0, w_ch1 = 0, w_ch2 = 0, w_q = 0, w_tq = 0, w_y = 0,
              w_dq = 0, w_d2 = 0, w_d1 = 0, w_dxa = 0, w_dhead = 0, w_e2z = 0, w_e2 = 0, w_e1 = 0, w_floats = 0;
};
// the layout of an accepted shape: n_critics critics of q_out outputs each (SAC: 1; TQC's quantile critics: n_quantiles, ev2g_tqc_host.h)
inline void sac_layout(SacPlan &p, int d_in, int h1, int h2, int d_out, int n_critics, int q_out) {
    p.d_in = d_in; p.h1 = h1; p.h2 = h2; p.d_out = d_out; p.nc = n_critics; p.da = d_in + d_out;
    const int ar[4] = {h1, h2, d_out, d_out}, ac[4] = {d_in, h1, h2, h2}, cr[3] = {h1, h2, q_out}, cc[3] = {p.da, h1, h2};
    for (int i = 0; i < 4; i++) { p.aoff[2 * i + 1] = p.aoff[2 * i] + ar[i] * ac[i]; p.aoff[2 * i + 2] = p.aoff[2 * i + 1] + ar[i]; }
    for (int i = 0; i < 3; i++) { p.coff[2 * i + 1] = p.coff[2 * i] + cr[i] * cc[i]; p.coff[2 * i + 2] = p.coff[2 * i + 1] + cr[i]; }
    p.n_actor = p.aoff[EV2G_SAC_ACTOR_ARRAYS]; p.n_critic = p.coff[6]; p.n_params = p.n_actor + p.nc * p.n_critic; p.head_block = d_out * h2 + d_out;
    p.k1 = mlp_round_up(d_in, 8); p.n1 = mlp_round_up(h1, 32); p.n2 = mlp_round_up(h2, 32); p.n3 = mlp_round_up(d_out, 32);
    const long long R = EV2G_TD3_MAX_BATCH;
    long long o = 0;
    auto take = [&o](long long n) { const long long at = o; o += n; return at; };
    p.w_xa = take(R * p.da); p.w_xb = take(R * p.da);
    p.w_ah1 = take(R * h1); p.w_ah2 = take(R * h2); p.w_head = take(2 * R * d_out); p.w_eps = take(R * d_out); p.w_a = take(R * d_out);
    p.w_lp = take(R); p.w_lp2 = take(R);
    p.w_ch1 = take(p.nc * R * h1); p.w_ch2 = take(p.nc * R * h2);
    p.w_q = take(p.nc * R * q_out); p.w_tq = take(p.nc * R * q_out); p.w_y = take(R); p.w_dq = take(p.nc * R * q_out);
    p.w_d2 = take(p.nc * R * h2); p.w_d1 = take(p.nc * R * h1); p.w_dxa = take(p.nc * R * d_out);
    p.w_dhead = take(2 * R * d_out); p.w_e2z = take(2 * R * h2); p.w_e2 = take(R * h2); p.w_e1 = take(R * h1);
    p.w_floats = o;
}
inline SacPlan plan_sac(int d_in, int h1, int h2, int d_out, int n_critics) {
    SacPlan p;
    auto refuse = [&p](const char *what, int v, int lo, int hi) {
        p.err = EV2G_ERR_ARG;
        p.refusal = std::string("ev2g_sac: ") + what + " " + std::to_string(v) + " is outside " + std::to_string(lo) + " .. " + std::to_string(hi);
        return p;
    };
    if (d_in < 1 || d_in > EV2G_SAC_MAX_IN) return refuse("d_in", d_in, 1, EV2G_SAC_MAX_IN);
    if (h1 < 1 || h1 > EV2G_SAC_MAX_HIDDEN) return refuse("h1", h1, 1, EV2G_SAC_MAX_HIDDEN);
    if (h2 < 1 || h2 > EV2G_SAC_MAX_HIDDEN) return refuse("h2", h2, 1, EV2G_SAC_MAX_HIDDEN);
    if (d_out < 1 || d_out > EV2G_SAC_MAX_OUT) return refuse("d_out", d_out, 1, EV2G_SAC_MAX_OUT);
    if (n_critics < 1 || n_critics > 2) return refuse("n_critics", n_critics, 1, 2);
    sac_layout(p, d_in, h1, h2, d_out, n_critics, 1);
    return p;
}
inline SacDev sac_dev(const SacPlan &p, float lo) {
    SacDev d{};
    d.d_in = p.d_in; d.h1 = p.h1; d.h2 = p.h2; d.d_out = p.d_out; d.k1 = p.k1; d.n1 = p.n1; d.n2 = p.n2; d.n3 = p.n3; d.lo = lo;
    return d;
}
// the six images' sizes in floats: w1, b1, w2, b2, wh, bh
inline void sac_image_sizes(const SacPlan &p, size_t out[6]) {
    out[0] = (size_t)p.n1 * p.k1; out[1] = (size_t)p.n1; out[2] = (size_t)p.n2 * p.n1; out[3] = (size_t)p.n2; out[4] = (size_t)2 * p.n3 * p.n2; out[5] = (size_t)2 * p.n3;
}

// ---- the config ----
inline void sac_default_config(ev2g_sac_config *c) {
    c->lr = 3e-4; c->beta1 = 0.9; c->beta2 = 0.999; c->adam_eps = 1e-8; c->tau = 0.005; c->gamma = 0.99;
    c->ent_coef = 1.0; c->target_entropy = 0.0;
    c->n_critics = 2; c->target_update_interval = 1; c->ent_coef_auto = 1; c->target_entropy_auto = 1;
}
inline std::vector<LearnerField> sac_rate_fields(double lr) { return {{"lr", lr, LEARNER_GE0}}; }
inline std::vector<LearnerField> sac_fields(const ev2g_sac_config &c) {
    std::vector<LearnerField> f = sac_rate_fields(c.lr);
    f.insert(f.end(), {{"beta1", c.beta1, LEARNER_UNIT}, {"beta2", c.beta2, LEARNER_UNIT}, {"adam_eps", c.adam_eps, LEARNER_GT0}, {"tau", c.tau, LEARNER_UNIT_CLOSED},
                       {"gamma", c.gamma, LEARNER_UNIT_CLOSED}, {"ent_coef", c.ent_coef, LEARNER_GT0},
                       {"target_entropy", c.target_entropy_auto ? 0.0 : std::fabs(c.target_entropy), LEARNER_GE0},   // (finite)
                       {"target_update_interval", (double)c.target_update_interval, LEARNER_GE1}});
    return f;
}
inline double sac_target_entropy(const ev2g_sac_config &c, int d_out) { return c.target_entropy_auto ? -(double)d_out : c.target_entropy; }

// ---- host twins of the element functions ----
// a [B, P] (tanh), a_env [B, P] (in [lo, 1]; may be null) and log pi [B] from mu, raw log_std and the draws' standard normals eps [B, P]; a row's
// eight partial sums are joined as the device's butterfly joins them
inline void sac_host_head(const float *mu, const float *log_std, const float *eps, int B, int P, float lo, float *a, float *a_env, float *logp) {
    for (int b = 0; b < B; b++) {
        double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int p = 0; p < P; p++) {
            const long long i = (long long)b * P + p;
            double t, lp;
            ev2g_sac_head_elem(mu[i], log_std[i], eps[i], &t, &lp);
            part[p & 7] += lp;
            a[i] = (float)t;
            if (a_env) a_env[i] = ev2g_sac_unscale_action((float)t, lo);
        }
        for (int s = 4; s >= 1; s >>= 1)
            for (int j = 0; j < s; j++) part[j] += part[j + s];
        logp[b] = (float)part[0];
    }
}
inline void sac_host_head_back(const float *mu, const float *log_std, const float *eps, const float *g, int B, int P, float log_alpha, float *d_mu,
                               float *d_log_std) {
    const double alpha = ev2g_sac_alpha(log_alpha), inv_b = 1.0 / (double)B;
    for (long long i = 0; i < (long long)B * P; i++) {
        double dm, dl;
        ev2g_sac_head_back_elem(mu[i], log_std[i], eps[i], (double)g[i], alpha, inv_b, &dm, &dl);
        d_mu[i] = (float)dm; d_log_std[i] = (float)dl;
    }
}
inline void sac_host_y(const float *tq, const float *logp, const float *reward, const uint8_t *done, int B, int nc, double gamma, float log_alpha, float *y) {
    const double alpha = ev2g_sac_alpha(log_alpha);
    for (int b = 0; b < B; b++) {
        float qm = tq[b];
        for (int j = 1; j < nc; j++) qm = fminf(qm, tq[(long long)j * B + b]);
        y[b] = ev2g_sac_y_elem(reward[b], done[b], gamma, qm, alpha, logp[b]);
    }
}
