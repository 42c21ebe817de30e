// ev2g_trpo_host.h -- the host-only half of the TRPO learner (ev2g_trpo.h): its config's checks, its LDS plan, the map of the actor's seven
// arrays, and the host twins of its conjugate-gradient iteration and of the line search's row terms.
//
// plan_trpo(widths) is plan_ppo's decision with the TRPO kernels' own LDS layout: one trunk at a time (the policy trunk in the policy step, the
// value trunk in the critic's gradient), the tangent blocks reused for the deltas, so the plan is never larger than PPO's for the same network
// and every network plan_ppo accepts is accepted.  The workspace is PPO's (the slabs of the thirteen arrays, of which a launch fills its own).
// trpo_map(plan, ppo map, direction images) says where element i of a flat actor vector -- log_std | pi_W1 | pi_b1 | pi_W2 | pi_b2 | action_W |
// action_b, sb3_contrib's order of the parameters without "value" in their name -- sits in the masters, the slabs and the direction images.
// Nothing here needs HIP or a handle (tests/host/trpo_check.cpp).
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "ev2g_policy_host.h"
#include "ev2g_learner_host.h"

#define EV2G_TRPO_ACTOR_ARRAYS 7
#define EV2G_TRPO_CG_BLOCK 1024   // threads of the one-workgroup vector kernels (conjugate gradient, step size, decide)

// what sb3_contrib's TRPO reads of its config, as the device stage keeps it
struct TrpoSpec {
    double lr = 1e-3, target_kl = 0.01, cg_damping = 0.1, shrink = 0.8;
    int cg_max_steps = 15, ls_max_iter = 10, normalize = 1;
};
inline TrpoSpec trpo_spec(const ev2g_trpo_config &c) {
    TrpoSpec s;
    s.lr = c.lr; s.target_kl = c.target_kl; s.cg_damping = c.cg_damping; s.shrink = c.line_search_shrinking_factor;
    s.cg_max_steps = c.cg_max_steps; s.ls_max_iter = c.line_search_max_iter; s.normalize = c.normalize_advantage ? 1 : 0;
    return s;
}
// the learner spine's view: the critic's optimiser is torch.optim.Adam(lr, 0.9, 0.999, eps 1e-5), which is what sb3_contrib's policy builds
inline LearnerSpec learner_spec(const ev2g_trpo_config &c) {
    LearnerSpec s;
    s.kind = LEARNER_TRPO;
    s.hyper = {0.0f, 1.0f, 0.0f, c.normalize_advantage ? 1 : 0};
    s.lr = c.lr; s.beta1 = 0.9; s.beta2 = 0.999; s.eps = 1e-5;
    s.grad_entry = "ev2g_trpo_grad";
    return s;
}
inline std::vector<LearnerField> trpo_rate_fields(double lr) { return {{"lr", lr, LEARNER_GE0}}; }
// (a shrinking factor in (0, 1): two rows of the table, > 0 and < 1)
inline std::vector<LearnerField> learner_fields(const ev2g_trpo_config &c) {
    std::vector<LearnerField> f = trpo_rate_fields(c.lr);
    f.insert(f.end(), {{"target_kl", c.target_kl, LEARNER_GT0}, {"cg_damping", c.cg_damping, LEARNER_GE0}, {"cg_max_steps", (double)c.cg_max_steps, LEARNER_GE1},
                       {"line_search_max_iter", (double)c.line_search_max_iter, LEARNER_GE1},
                       {"line_search_shrinking_factor", c.line_search_shrinking_factor, LEARNER_GT0},
                       {"line_search_shrinking_factor", c.line_search_shrinking_factor, LEARNER_UNIT}});
    return f;
}

// ---- the LDS plan: offsets in floats from the 16-byte aligned base.  The first 6 n3 floats are three float64 arrays of n3: exp(-2 log_std), and
// the line search's per-port constants kc and kq (ev2g_trpo_kl_consts).  A: a trunk's first hidden layer, B: its second (strides of the wider
// trunk); T1 / T2: the tangents, then the deltas, of A / B.
struct TrpoLds {
    int sX, sA, sB, sMU;
    int oIV, oKC, oKQ, oX, oH1, oH2, oT1, oT2, oMU, oACT, oROW;
    size_t bytes;
};
constexpr TrpoLds trpo_lds(int k1r, int n1, int n2, int m1, int m2, int n3) {
    TrpoLds l{};
    const int R = EV2G_PPO_ROWS;
    l.sX = k1r + 4; l.sA = (n1 > m1 ? n1 : m1) + 4; l.sB = (n2 > m2 ? n2 : m2) + 4; l.sMU = n3 + 4;
    int o = 0;
    l.oIV = o; o += 2 * n3;
    l.oKC = o; o += 2 * n3;
    l.oKQ = o; o += 2 * n3;
    l.oX = o; o += R * l.sX;
    l.oH1 = o; o += R * l.sA;
    l.oH2 = o; o += R * l.sB;
    l.oT1 = o; o += R * l.sA;
    l.oT2 = o; o += R * l.sB;
    l.oMU = o; o += R * l.sMU;
    l.oACT = o; o += R * l.sMU;
    l.oROW = o; o += 3 * R;
    l.bytes = (size_t)o * sizeof(float);
    return l;
}

struct TrpoPlan {
    int err = EV2G_OK;
    std::string refusal;
    PpoPlan ppo{};                    // the arrays' offsets, the slabs, the grid cap, the workspace: PPO's
    TrpoLds lds{};
    int n_actor = 0;                  // elements of a flat actor vector
    int arr[EV2G_TRPO_ACTOR_ARRAYS] = {}, off[EV2G_TRPO_ACTOR_ARRAYS + 1] = {};   // the seven arrays as rows of ac_params, and where each starts
    size_t vector_bytes = 0;          // the conjugate-gradient state: g, x, r, p, Hv in float64 and theta0 in float32
};
inline TrpoPlan plan_trpo(int d_in, int h1, int h2, int v1, int v2, int d_out) {
    TrpoPlan t;
    t.ppo = plan_ppo(d_in, h1, h2, v1, v2, d_out);
    if (t.ppo.err) { t.err = t.ppo.err; t.refusal = t.ppo.refusal; return t; }
    const AcPlan &a = t.ppo.ac;
    t.lds = trpo_lds(t.ppo.k1r, a.n1, a.n2, a.m1, a.m2, a.n3);
    static const int order[EV2G_TRPO_ACTOR_ARRAYS] = {12, 0, 1, 2, 3, 8, 9};   // log_std, pi_W1, pi_b1, pi_W2, pi_b2, action_W, action_b
    int o = 0;
    for (int k = 0; k < EV2G_TRPO_ACTOR_ARRAYS; k++) { t.arr[k] = order[k]; t.off[k] = o; o += t.ppo.rows[order[k]] * t.ppo.cols[order[k]]; }
    t.off[EV2G_TRPO_ACTOR_ARRAYS] = o; t.n_actor = o;
    t.vector_bytes = (size_t)o * (5 * sizeof(double) + sizeof(float));
    return t;
}

// where element i of a flat actor vector sits.  dimg: the direction images of the Fisher product (pack_linear_f32 order for the three matrices,
// padded vectors for the three biases, null for log_std) -- the same sizes and packing as the policy's own six images.
struct TrpoMap {
    int off[EV2G_TRPO_ACTOR_ARRAYS + 1], arr[EV2G_TRPO_ACTOR_ARRAYS], cols[EV2G_TRPO_ACTOR_ARRAYS], img_k[EV2G_TRPO_ACTOR_ARRAYS];
    int n_actor;
    float *dimg[EV2G_TRPO_ACTOR_ARRAYS];
};
inline TrpoMap trpo_map(const TrpoPlan &pl, float *const dimg[EV2G_TRPO_ACTOR_ARRAYS]) {
    TrpoMap m{};
    const auto tab = ac_params(pl.ppo.ac);
    for (int k = 0; k < EV2G_TRPO_ACTOR_ARRAYS; k++) {
        m.off[k] = pl.off[k]; m.arr[k] = pl.arr[k]; m.cols[k] = pl.ppo.cols[pl.arr[k]]; m.img_k[k] = tab[(size_t)pl.arr[k]].img_k; m.dimg[k] = dimg[k];
    }
    m.off[EV2G_TRPO_ACTOR_ARRAYS] = pl.off[EV2G_TRPO_ACTOR_ARRAYS]; m.n_actor = pl.n_actor;
    return m;
}

// the state of one policy step, on the device: what the queued launches read to know whether they still have work
struct TrpoState {
    int cg_done, cg_iters, ls_done, ls_tries, accepted, failed, pad0, pad1;
    double rho, J0, J1, kl, beta, c, xHx;
};

#include "ev2g_trpo.h"

// ---- host twins ----
// one iteration of the conjugate-gradient vector algebra from a given Hp (ev2g_host_trpo_cg_step): x += alpha p; unless `last`: r -= alpha Hp,
// rho' = r . r, and unless rho' < 1e-10: p = r + (rho' / rho) p rounded to float32 (the device's product reads p's float32 image).  Dots in float64,
// elements ascending.  Returns 1 when the solve has ended.
inline int trpo_host_cg_step(double *x, double *r, double *p, const double *Hp, int n, double *rho, int last) {
    double pHp = 0.0;
    for (int i = 0; i < n; i++) pHp += p[i] * Hp[i];
    const double alpha = *rho / pHp;
    for (int i = 0; i < n; i++) x[i] += alpha * p[i];
    if (last) return 1;
    double rn = 0.0;
    for (int i = 0; i < n; i++) { r[i] -= alpha * Hp[i]; rn += r[i] * r[i]; }
    if (rn < EV2G_TRPO_RHO_MIN) { *rho = rn; return 1; }
    const double b = rn / *rho;
    for (int i = 0; i < n; i++) p[i] = (double)(float)(r[i] + b * p[i]);   // (p stays float32-representable, as on the device)
    *rho = rn;
    return 0;
}

// the row terms of J and KL (ev2g_host_trpo_rows): j[i] = A^_i exp(lp_i - old_lp_i), kl[i] = sum_p KL(N(mean_ip, e^{ls_p}) || N(mean0_ip, e^{ls0_p})),
// a row's sums over eight partial sums joined as the device's butterfly joins them
inline void trpo_host_rows(const float *mean, const float *mean0, const float *actions, const float *log_std, const float *log_std0, const float *old_lp,
                           const float *adv, int B, int P, int normalize, double *j, double *kl) {
    double a_mean = 0.0, a_scale = 1.0;
    const bool norm = normalize && B > 1;
    if (norm) {
        double s = 0.0;
        for (int i = 0; i < B; i++) s += (double)adv[i];
        a_mean = s / B;
        s = 0.0;
        for (int i = 0; i < B; i++) { const double d = (double)adv[i] - a_mean; s += d * d; }
        a_scale = 1.0 / (std::sqrt(s / (double)(B - 1)) + 1e-8);
    }
    std::vector<double> iv((size_t)P), kc((size_t)P), kq((size_t)P);
    for (int p = 0; p < P; p++) {
        iv[(size_t)p] = std::exp(-2.0 * (double)log_std[p]);
        ev2g_trpo_kl_consts(log_std[p], log_std0[p], &kc[(size_t)p], &kq[(size_t)p]);
    }
    for (int i = 0; i < B; i++) {
        const float *mu = mean + (size_t)i * P, *mu0 = mean0 + (size_t)i * P, *a = actions + (size_t)i * P;
        double q[8], k[8];
        for (int jj = 0; jj < 8; jj++) {
            q[jj] = ev2g_ppo_lp_part(mu, a, log_std, iv.data(), P, jj, 8);
            k[jj] = ev2g_trpo_kl_part(mu, mu0, kc.data(), kq.data(), P, jj, 8);
        }
        const float A = norm ? (float)(((double)adv[i] - a_mean) * a_scale) : adv[i];
        j[i] = (double)A * std::exp(ev2g_ppo_join8(q) - (double)old_lp[i]);
        kl[i] = ev2g_ppo_join8(k);
    }
}
