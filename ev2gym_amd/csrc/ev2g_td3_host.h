// ev2g_td3_host.h -- the host-only half of the TD3 / DDPG learner (ev2g_td3.h): which networks and batches it accepts, where every parameter
// array and every workspace block sits, the config's checks, and the host twins of its element functions.
//
// plan_td3(d_in, h1, h2, d_out, n_critics) refuses with one message per field, as plan_ac / plan_ppo do, and lays out
//   * the flat parameter buffer (masters, targets, Adam's m and v, the gradient: the same layout): the actor's W1 | b1 | W2 | b2 | W3 | b3 in
//     SB3's [out, in] layout, then the same six arrays of critic 0, then critic 1 -- SB3's parameter order (actor.mu.{0,2,4}, critic.qf{0,1}.{0,2,4});
//   * the workspace of one batch of EV2G_TD3_MAX_BATCH rows (offsets in floats).
// td3_fields is the config's list for learner_refusal (ev2g_learner_host.h).  Nothing here needs HIP or a handle: tests/host/td3_check.cpp
// enumerates it.
#pragma once
#include <string>
#include <vector>

#include "../../include/ev2g.h"
#include "ev2g_learner_host.h"
#include "ev2g_td3.h"

#define EV2G_TD3_MAX_IN 192
#define EV2G_TD3_MAX_OUT 64
#define EV2G_TD3_MAX_HIDDEN 400
static_assert(EV2G_TD3_MAX_BATCH == 1024, "ev2g_replay_stream_index strides a draw's rows by 1024");

struct Td3Plan {
    int err = EV2G_OK;
    std::string refusal;
    int d_in = 0, h1 = 0, h2 = 0, d_out = 0, nc = 0, da = 0;   // da = d_in + d_out: a critic's input width
    int aoff[7] = {}, coff[7] = {};   // the six arrays' starts inside the actor's / one critic's block ([6]: the block's size)
    int n_actor = 0, n_critic = 0, n_params = 0;   // n_params = n_actor + nc * n_critic; critic j's block starts at n_actor + j * n_critic
    // workspace (floats): critic input (s, a~) | (s', a') or (s, actor(s)) | the actor's h1, h2, output | per critic h1, h2 | values q, target
    // values tq [nc, B] | y [B] | dq [nc, B] | per critic deltas d2, d1 | the actor's deltas e2, e1, its output delta dmu | d(xa) action columns
    long long w_xa = 0, w_xb = 0, w_ah1 = 0, w_ah2 = 0, w_amu = 0, w_ch1 = 0, w_ch2 = 0, w_q = 0, w_tq = 0, w_y = 0, w_dq = 0, w_d2 = 0, w_d1 = 0, w_e2 = 0,
              w_e1 = 0, w_dmu = 0, w_floats = 0;
};
inline Td3Plan plan_td3(int d_in, int h1, int h2, int d_out, int n_critics) {
    Td3Plan p;
    auto refuse = [&p](const char *what, int v, int lo, int hi) {
        p.err = EV2G_ERR_ARG;
        p.refusal = std::string("ev2g_td3: ") + what + " " + std::to_string(v) + " is outside " + std::to_string(lo) + " .. " + std::to_string(hi);
        return p;
    };
    if (d_in < 1 || d_in > EV2G_TD3_MAX_IN) return refuse("d_in", d_in, 1, EV2G_TD3_MAX_IN);
    if (h1 < 1 || h1 > EV2G_TD3_MAX_HIDDEN) return refuse("h1", h1, 1, EV2G_TD3_MAX_HIDDEN);
    if (h2 < 1 || h2 > EV2G_TD3_MAX_HIDDEN) return refuse("h2", h2, 1, EV2G_TD3_MAX_HIDDEN);
    if (d_out < 1 || d_out > EV2G_TD3_MAX_OUT) return refuse("d_out", d_out, 1, EV2G_TD3_MAX_OUT);
    if (n_critics < 1 || n_critics > 2) return refuse("n_critics", n_critics, 1, 2);
    p.d_in = d_in; p.h1 = h1; p.h2 = h2; p.d_out = d_out; p.nc = n_critics; p.da = d_in + d_out;
    const int ar[3] = {h1, h2, d_out}, ac[3] = {d_in, h1, h2}, cr[3] = {h1, h2, 1}, cc[3] = {p.da, h1, h2};
    for (int i = 0; i < 3; i++) {
        p.aoff[2 * i + 1] = p.aoff[2 * i] + ar[i] * ac[i]; p.aoff[2 * i + 2] = p.aoff[2 * i + 1] + ar[i];
        p.coff[2 * i + 1] = p.coff[2 * i] + cr[i] * cc[i]; p.coff[2 * i + 2] = p.coff[2 * i + 1] + cr[i];
    }
    p.n_actor = p.aoff[6]; p.n_critic = p.coff[6]; p.n_params = p.n_actor + p.nc * p.n_critic;
    const long long R = EV2G_TD3_MAX_BATCH;
    long long o = 0;
    auto take = [&o](long long n) { const long long at = o; o += n; return at; };
    p.w_xa = take(R * p.da); p.w_xb = take(R * p.da);
    p.w_ah1 = take(R * h1); p.w_ah2 = take(R * h2); p.w_amu = take(R * d_out);
    p.w_ch1 = take(p.nc * R * h1); p.w_ch2 = take(p.nc * R * h2);
    p.w_q = take(p.nc * R); p.w_tq = take(p.nc * R); p.w_y = take(R); p.w_dq = take(p.nc * R);
    p.w_d2 = take(p.nc * R * h2); p.w_d1 = take(p.nc * R * h1);
    p.w_e2 = take(R * h2); p.w_e1 = take(R * h1); p.w_dmu = take(R * d_out);
    p.w_floats = o;
    return p;
}
// the batch size every gradient entry checks
inline std::string td3_batch_refusal(const char *who, int B) {
    if (B >= 1 && B <= EV2G_TD3_MAX_BATCH) return std::string();
    return std::string(who) + ": B " + std::to_string(B) + " is outside 1 .. " + std::to_string(EV2G_TD3_MAX_BATCH);
}

// ---- the config ----
inline void td3_default_config(int ddpg, ev2g_td3_config *c) {
    c->lr = 1e-3; c->beta1 = 0.9; c->beta2 = 0.999; c->adam_eps = 1e-8; c->tau = 0.005; c->gamma = 0.99;
    c->target_policy_noise = ddpg ? 0.0 : 0.2; c->target_noise_clip = 0.5;
    c->n_critics = ddpg ? 1 : 2; c->policy_delay = ddpg ? 1 : 2;
}
inline std::vector<LearnerField> td3_rate_fields(double lr) { return {{"lr", lr, LEARNER_GE0}}; }
inline std::vector<LearnerField> td3_fields(const ev2g_td3_config &c) {
    std::vector<LearnerField> f = td3_rate_fields(c.lr);
    f.insert(f.end(), {{"beta1", c.beta1, LEARNER_UNIT}, {"beta2", c.beta2, LEARNER_UNIT}, {"adam_eps", c.adam_eps, LEARNER_GT0}, {"tau", c.tau, LEARNER_UNIT_CLOSED},
                       {"gamma", c.gamma, LEARNER_UNIT_CLOSED}, {"target_policy_noise", c.target_policy_noise, LEARNER_GE0},
                       {"target_noise_clip", c.target_noise_clip, LEARNER_GE0}, {"policy_delay", (double)c.policy_delay, LEARNER_GE1}});
    return f;
}

// ---- host twins of the element functions ----
// a' [B, P] and y [B] from the target actor's output a_target [B, P], the standard normals of the draws (normals [B, P]; not read when sigma is
// 0), the target critics' values tq [nc, B] computed on (s', a') by the caller, reward and done
inline void td3_host_smooth(const float *a_target, const float *normals, long long n, double sigma, double clip, float *a_next) {
    for (long long i = 0; i < n; i++) a_next[i] = ev2g_td3_smooth_elem(a_target[i], sigma > 0.0 ? normals[i] : 0.0f, (float)sigma, (float)clip);
}
inline void td3_host_y(const float *tq, const float *reward, const uint8_t *done, int B, int nc, double gamma, float *y) {
    for (int b = 0; b < B; b++) {
        float qm = tq[b];
        for (int j = 1; j < nc; j++) qm = fminf(qm, tq[(long long)j * B + b]);
        y[b] = ev2g_td3_y_elem(reward[b], done[b], (float)gamma, qm);
    }
}
inline void td3_host_polyak(float *target, const float *param, long long n, double tau) {
    for (long long i = 0; i < n; i++) target[i] = ev2g_polyak_elem(target[i], param[i], (float)(1.0 - tau), (float)tau);
}
