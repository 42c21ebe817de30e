// ev2g_tqc_host.h -- the host-only half of the TQC learner (ev2g_tqc.h): which networks and quantile settings it accepts, where every parameter
// array and every workspace block sits, the config's checks, and the host twins of the distributional kernels.
//
// plan_tqc(d_in, h1, h2, d_out, n_critics, n_quantiles, top_quantiles_to_drop) refuses with one message per field, in plan_sac's wording, and lays
// out a SacPlan (ev2g_sac_host.h: sac_layout) whose critics have n_quantiles outputs:
//   * the flat parameter buffer: the actor's eight arrays, then the six arrays of critic 0, 1, ... -- sb3_contrib's parameter order
//     (actor.latent_pi.{0,2}, actor.mu, actor.log_std, critic.qf{j}.{0,2,4}); the targets are the critics' blocks alone, in the same order;
//   * SAC's workspace with q, tq and dq as [nc][B, nq] and the per-critic blocks for up to five critics, then z [B, K], the per-row float64
//     partials [B] (an even offset: 8-byte aligned) and the summed input deltas [B, P].
// The limits: D <= 192, hidden widths 1 .. 256, P <= 64 (the collection kernel's), n_critics 1 .. 5, n_quantiles 1 .. 64, at most 128 pooled atoms
// (the sorting network's width), 0 <= drop with at least one atom kept.  Nothing here needs HIP or a handle: tests/host/tqc_check.cpp enumerates it.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "ev2g_sac_host.h"
#include "ev2g_tqc.h"

struct TqcPlan : SacPlan {
    int nq = 0, drop = 0, M = 0, K = 0;            // quantiles per critic, atoms dropped per critic, pooled atoms nc nq, kept atoms M - drop nc
    long long w_z = 0, w_part = 0, w_g = 0;        // z [B, K] | the rows' float64 partials [B] (2 floats each) | sum_j of the critics' input deltas [B, P]
};
inline TqcPlan plan_tqc(int d_in, int h1, int h2, int d_out, int n_critics, int n_quantiles, int top_quantiles_to_drop) {
    TqcPlan p;
    auto refuse = [&p](const char *what, int v, int lo, int hi) {
        p.err = EV2G_ERR_ARG;
        p.refusal = std::string("ev2g_tqc: ") + what + " " + std::to_string(v) + " is outside " + std::to_string(lo) + " .. " + std::to_string(hi);
        return p;
    };
    if (d_in < 1 || d_in > EV2G_SAC_MAX_IN) return refuse("d_in", d_in, 1, EV2G_SAC_MAX_IN);
    if (h1 < 1 || h1 > EV2G_SAC_MAX_HIDDEN) return refuse("h1", h1, 1, EV2G_SAC_MAX_HIDDEN);
    if (h2 < 1 || h2 > EV2G_SAC_MAX_HIDDEN) return refuse("h2", h2, 1, EV2G_SAC_MAX_HIDDEN);
    if (d_out < 1 || d_out > EV2G_SAC_MAX_OUT) return refuse("d_out", d_out, 1, EV2G_SAC_MAX_OUT);
    if (n_critics < 1 || n_critics > EV2G_TQC_MAX_CRITICS) return refuse("n_critics", n_critics, 1, EV2G_TQC_MAX_CRITICS);
    if (n_quantiles < 1 || n_quantiles > EV2G_TQC_MAX_QUANTILES) return refuse("n_quantiles", n_quantiles, 1, EV2G_TQC_MAX_QUANTILES);
    if (n_critics * n_quantiles > EV2G_TQC_MAX_ATOMS) return refuse("n_critics * n_quantiles", n_critics * n_quantiles, 1, EV2G_TQC_MAX_ATOMS);
    // K = n_critics (n_quantiles - drop) >= 1
    if (top_quantiles_to_drop < 0 || top_quantiles_to_drop > n_quantiles - 1)
        return refuse("top_quantiles_to_drop_per_net", top_quantiles_to_drop, 0, n_quantiles - 1);
    sac_layout(p, d_in, h1, h2, d_out, n_critics, n_quantiles);
    p.nq = n_quantiles; p.drop = top_quantiles_to_drop; p.M = n_critics * n_quantiles; p.K = p.M - top_quantiles_to_drop * n_critics;
    const long long R = EV2G_TD3_MAX_BATCH;
    p.w_z = p.w_floats;
    p.w_part = p.w_z + R * p.K; p.w_part += p.w_part & 1;
    p.w_g = p.w_part + 2 * R;
    p.w_floats = p.w_g + R * d_out;
    return p;
}

// ---- the config ----
inline void tqc_default_config(ev2g_tqc_config *c) {
    c->lr = 3e-4; c->beta1 = 0.9; c->beta2 = 0.999; c->adam_eps = 1e-8; c->tau = 0.005; c->gamma = 0.99;
    c->ent_coef = 1.0; c->target_entropy = 0.0;
    c->n_critics = 2; c->target_update_interval = 1; c->ent_coef_auto = 1; c->target_entropy_auto = 1;
    c->n_quantiles = 25; c->top_quantiles_to_drop_per_net = 2;
}
// the fields TQC shares with SAC, as SAC's config: what the shared actor side, the optimiser steps and the Polyak step read
inline ev2g_sac_config tqc_sac_config(const ev2g_tqc_config &c) {
    ev2g_sac_config s;
    s.lr = c.lr; s.beta1 = c.beta1; s.beta2 = c.beta2; s.adam_eps = c.adam_eps; s.tau = c.tau; s.gamma = c.gamma; s.ent_coef = c.ent_coef;
    s.target_entropy = c.target_entropy; s.n_critics = c.n_critics; s.target_update_interval = c.target_update_interval; s.ent_coef_auto = c.ent_coef_auto;
    s.target_entropy_auto = c.target_entropy_auto;
    return s;
}
inline std::vector<LearnerField> tqc_fields(const ev2g_tqc_config &c) { return sac_fields(tqc_sac_config(c)); }

// ---- host twins of the distributional kernels ----
// sum over i < n of f(i) in ev2g_td3_block_sum's order: 256 strided partials, i ascending within one, joined in thread order
template <class F>
inline double tqc_host_block_sum(int n, F f) {
    double part[256];
    for (int t = 0; t < 256; t++) part[t] = 0.0;
    for (int i = 0; i < n; i++) part[i & 255] += f(i);
    double s = 0.0;
    for (int t = 0; t < 256; t++) s += part[t];
    return s;
}
// the K smallest of a row's M pooled atoms v (pool order) under ev2g_tqc_key_less, ascending, into out [K]: what the device's network leaves
inline void tqc_host_sort_row(const float *v, int M, int K, float *out) {
    std::vector<int> idx((size_t)M);
    for (int m = 0; m < M; m++) idx[(size_t)m] = m;
    std::sort(idx.begin(), idx.end(), [v](int a, int b) { return ev2g_tqc_key_less(v[a], a, v[b], b); });
    for (int k = 0; k < K; k++) out[k] = v[idx[(size_t)k]];
}
// z [B, K] from the target critics' atoms tq [nc][B, nq] and log pi' [B]
inline void tqc_host_target(const float *tq, const float *logp, const float *reward, const uint8_t *done, int B, int nc, int nq, int drop, double gamma,
                            float log_alpha, float *z) {
    const int M = nc * nq, K = M - drop * nc;
    const double alpha = ev2g_sac_alpha(log_alpha);
    std::vector<float> pool((size_t)M), kept((size_t)K);
    for (int b = 0; b < B; b++) {
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nq; i++) pool[(size_t)(j * nq + i)] = tq[((long long)j * B + b) * nq + i];
        tqc_host_sort_row(pool.data(), M, K, kept.data());
        for (int k = 0; k < K; k++) z[(long long)b * K + k] = ev2g_sac_y_elem(reward[b], done[b], gamma, kept[(size_t)k], alpha, logp[b]);
    }
}
// dq [nc][B, nq] and the critic loss from z [B, K] and q [nc][B, nq]: the device's chains and joins
inline float tqc_host_critic_head(const float *z, const float *q, int B, int nc, int nq, int K, float *dq) {
    const double inv_terms = ev2g_tqc_inv_terms(B, nc, nq, K);
    std::vector<double> part((size_t)B);
    for (int b = 0; b < B; b++) {
        double s = 0.0;
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nq; i++) {
                const long long at = ((long long)j * B + b) * nq + i;
                const double tau = ev2g_tqc_tau(i, nq);
                double g = 0.0, l = 0.0;
                for (int k = 0; k < K; k++) ev2g_tqc_pair(z[(long long)b * K + k], q[at], tau, &g, &l);
                dq[at] = ev2g_tqc_dq_elem(g, inv_terms);
                s += l;
            }
        part[(size_t)b] = s;
    }
    return (float)(tqc_host_block_sum(B, [&](int b) { return part[(size_t)b]; }) * inv_terms);
}
// the actor's head on q [nc][B, nq] = critic_j(s, a_pi) and log pi [B]: out4 = {actor_loss, ent_coef_loss, alpha, the gradient of log_ent_coef}
inline void tqc_host_actor_head(const float *q, const float *logp, int B, int nc, int nq, float log_alpha, double target_entropy, int auto_alpha, float *out4) {
    const double inv_b = 1.0 / (double)B, la = (double)log_alpha, alpha = ev2g_sac_alpha(log_alpha), inv_m = 1.0 / ((double)nc * (double)nq);
    std::vector<double> part((size_t)B);
    for (int b = 0; b < B; b++) {
        double s = 0.0;
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nq; i++) s += (double)q[((long long)j * B + b) * nq + i];
        part[(size_t)b] = s;
    }
    const double s1 = tqc_host_block_sum(B, [&](int b) { return alpha * (double)logp[b] - part[(size_t)b] * inv_m; });
    const double s2 = tqc_host_block_sum(B, [&](int b) { return (double)logp[b] + target_entropy; });
    const double g = -(s2 * inv_b);
    out4[0] = (float)(s1 * inv_b);
    out4[1] = auto_alpha ? (float)(la * g) : 0.0f;
    out4[2] = (float)alpha;
    out4[3] = auto_alpha ? (float)g : 0.0f;
}
