// ev2g_ars_host.h -- the host-only half of the ARS learner (ev2g_ars.h; sb3_contrib's ARS, Augmented Random Search): which policies it accepts,
// where every element of theta sits in a candidate's packed image, the row -> (candidate, tile) map of the population actor, the LDS bytes, the
// byte budget, the config's checks, and the host twins of the perturb, returns and update launches.
//
//   MlpPolicy     obs[D] -> ReLU(h1) -> ReLU(h2) -> linear(P) -> tanh -> the env's box [lo, 1];   theta = W1 | b1 | W2 | b2 | W3 | b3
//   LinearPolicy  obs[D] -> linear(P), no bias, clipped to [lo, 1];                               theta = W
// every matrix [out, in] row-major (torch's parameters_to_vector).  A candidate's image is the layers' pack_linear_f32 images and zero-padded
// biases one behind the other (the linear policy: the matrix and a bias block that stays zero); candidate c's starts c * stride floats behind
// the first one's.  Padding is zeroed at create and never addressed afterwards: ars_image_index maps only the elements of theta.
//
// One iteration on 2 n_delta candidates (k: theta + delta_std delta_k, n_delta + k: theta - delta_std delta_k) whose returns are r[c]:
//   score_k = max(r+_k, r-_k); rank: score descending, ties to the lower k (by counting); the n_top best directions are kept, in rank order;
//   sigma_R = the unbiased standard deviation of r+ of the kept directions in rank order, then r- likewise (two passes, float64);
//   step = learning_rate / (n_top sigma_R + 1e-6);   theta_i <- (float)((double)theta_i + step * sum_j (r+_j - r-_j) (double)delta_j,i), j in rank order.
// A return that is not finite refuses the update: theta keeps its bits, the report carries the flag and the first such candidate.
// Nothing here needs HIP or a handle: tests/host/ars_check.cpp enumerates it (it defines __host__ and __device__ to nothing).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ev2g.h"
#include "ev2g_learner_host.h"
#include "ev2g_policy_host.h"
#include "ev2g_sac.h"   // ev2g_sac_unscale_action, ev2g_sac_lds_max

#define EV2G_ARS_MAX_DELTA 4096
#define EV2G_ARS_ARRAYS 6

// where theta's arrays start (off), their row length (cols; 0: a vector), and where each one's image starts inside a candidate's image (img) with
// the padded input width its matrix is packed for (img_k).  Passed to the kernels by value.
struct ArsLayout {
    int n_arrays, n_params;
    int off[EV2G_ARS_ARRAYS + 1], cols[EV2G_ARS_ARRAYS], img[EV2G_ARS_ARRAYS], img_k[EV2G_ARS_ARRAYS];
};
// the position of theta_i inside a candidate's image
__host__ __device__ inline long long ars_image_index(const ArsLayout &L, int i) {
    int a = 0;
    while (a + 1 < L.n_arrays && i >= L.off[a + 1]) a++;
    const int e = i - L.off[a];
    if (L.cols[a] == 0) return (long long)L.img[a] + e;
    return (long long)L.img[a] + (long long)packed_f32_index(e / L.cols[a], e % L.cols[a], L.img_k[a]);
}

// the population actor's network: widths, padded widths (inputs to 8, columns to 32; the linear policy: n1 = n2 = 0), where the layers' images
// start inside a candidate's image, and the candidates' stride (floats)
struct ArsDev {
    int kind, d_in, h1, h2, d_out;
    int k1, n1, n2, n3;
    float lo;
    int o_w1, o_b1, o_w2, o_b2, o_w3, o_b3;
    long long stride;
};
struct ArsLds { int sA, sB; size_t bytes; };
// two activation blocks of 32 rows (float32, +16 bytes per row): A the input rows, then the second hidden layer; B the first, then the head
__host__ __device__ inline ArsLds ev2g_ars_lds(const ArsDev &m) {
    ArsLds l;
    l.sA = (m.k1 > m.n2 ? m.k1 : m.n2) + 4; l.sB = (m.n1 > m.n3 ? m.n1 : m.n3) + 4;
    l.bytes = (size_t)32 * (l.sA + l.sB) * sizeof(float);
    return l;
}

// workgroup b of a population launch of C candidates x R rows: its candidate, its first row and its live rows
struct ArsTile { int cand; long long row0; int live; };
__host__ __device__ inline int ars_tiles_per_candidate(int R) { return (R + 31) / 32; }
__host__ __device__ inline ArsTile ars_tile_of(int b, int R) {
    const int tpc = ars_tiles_per_candidate(R), c = b / tpc, t = b - c * tpc;
    ArsTile o;
    o.cand = c; o.row0 = (long long)c * R + 32ll * t; o.live = R - 32 * t < 32 ? R - 32 * t : 32;
    return o;
}

struct ArsPlan {
    int err = EV2G_OK;
    std::string refusal;
    int kind = 0, n_delta = 0, n_top = 0;
    ArsLayout lay{};
    ArsDev dev{};
    size_t lds = 0;
    // bytes: theta, the centre image and the 2 n_delta candidate images, the directions [n_delta, n_params], the returns, ranks and report
    size_t image_bytes = 0, delta_bytes = 0, state_bytes = 0, total_bytes = 0;
};

inline std::vector<LearnerField> ars_rate_fields(double lr, double delta_std) { return {{"learning_rate", lr, LEARNER_GE0}, {"delta_std", delta_std, LEARNER_GT0}}; }
inline void ars_default_config(ev2g_ars_config *c) {
    c->learning_rate = 0.02; c->delta_std = 0.05; c->alive_bonus_offset = 0.0; c->n_delta = 8; c->n_top = 8;
}
// the EV2G_ERR_ARG message of the first config rule broken, or empty
inline std::string ars_config_refusal(const char *who, const ev2g_ars_config &c) {
    std::string r = learner_refusal(who, ars_rate_fields(c.learning_rate, c.delta_std));
    if (!r.empty()) return r;
    if (!std::isfinite(c.alive_bonus_offset)) return std::string(who) + ": alive_bonus_offset must be finite";
    if (c.n_delta < 1 || c.n_delta > EV2G_ARS_MAX_DELTA) return std::string(who) + ": n_delta " + std::to_string(c.n_delta) + " is outside 1 .. " + std::to_string(EV2G_ARS_MAX_DELTA);
    if (c.n_top < 1 || c.n_top > c.n_delta) return std::string(who) + ": n_top " + std::to_string(c.n_top) + " is outside 1 .. n_delta (" + std::to_string(c.n_delta) + ")";
    return std::string();
}
// a rollout's env count: a positive multiple of 2 n_delta
inline std::string ars_rows_refusal(const char *who, const char *what, long long n, int n_delta) {
    if (n >= 1 && n % (2ll * n_delta) == 0) return std::string();
    return std::string(who) + ": " + what + " " + std::to_string(n) + " is not a positive multiple of 2 n_delta (" + std::to_string(2 * n_delta) + ")";
}

inline ArsPlan plan_ars(int kind, int d_in, int h1, int h2, int d_out, int n_delta, int n_top) {
    ArsPlan p;
    auto refuse = [&p](const std::string &why) { p.err = EV2G_ERR_ARG; p.refusal = why; return p; };
    auto range = [](const char *what, int v, int hi) { return std::string("ev2g_ars: ") + what + " " + std::to_string(v) + " is outside 1 .. " + std::to_string(hi); };
    if (kind != EV2G_ARS_MLP && kind != EV2G_ARS_LINEAR) return refuse("ev2g_ars: kind must be EV2G_ARS_MLP or EV2G_ARS_LINEAR");
    if (d_in < 1 || d_in > EV2G_AC_MAX_IN) return refuse(range("d_in", d_in, EV2G_AC_MAX_IN));
    if (kind == EV2G_ARS_MLP) {
        if (h1 < 1 || h1 > EV2G_AC_MAX_HIDDEN) return refuse(range("h1", h1, EV2G_AC_MAX_HIDDEN));
        if (h2 < 1 || h2 > EV2G_AC_MAX_HIDDEN) return refuse(range("h2", h2, EV2G_AC_MAX_HIDDEN));
    }
    if (d_out < 1 || d_out > EV2G_AC_MAX_OUT) return refuse(range("d_out", d_out, EV2G_AC_MAX_OUT));
    if (n_delta < 1 || n_delta > EV2G_ARS_MAX_DELTA) return refuse(range("n_delta", n_delta, EV2G_ARS_MAX_DELTA));
    if (n_top < 1 || n_top > n_delta) return refuse("ev2g_ars: n_top " + std::to_string(n_top) + " is outside 1 .. n_delta (" + std::to_string(n_delta) + ")");
    p.kind = kind; p.n_delta = n_delta; p.n_top = n_top;
    ArsDev &d = p.dev;
    ArsLayout &L = p.lay;
    d.kind = kind; d.d_in = d_in; d.d_out = d_out; d.lo = -1.0f;
    d.k1 = mlp_round_up(d_in, 8); d.n3 = mlp_round_up(d_out, 32);
    if (kind == EV2G_ARS_MLP) {
        d.h1 = h1; d.h2 = h2; d.n1 = mlp_round_up(h1, 32); d.n2 = mlp_round_up(h2, 32);
        d.o_w1 = 0; d.o_b1 = d.o_w1 + d.n1 * d.k1; d.o_w2 = d.o_b1 + d.n1; d.o_b2 = d.o_w2 + d.n2 * d.n1; d.o_w3 = d.o_b2 + d.n2; d.o_b3 = d.o_w3 + d.n3 * d.n2;
        d.stride = (long long)d.o_b3 + d.n3;
        const int rows[6] = {h1, h1, h2, h2, d_out, d_out}, cols[6] = {d_in, 0, h1, 0, h2, 0};
        const int img[6] = {d.o_w1, d.o_b1, d.o_w2, d.o_b2, d.o_w3, d.o_b3}, img_k[6] = {d.k1, 0, d.n1, 0, d.n2, 0};
        L.n_arrays = 6;
        for (int i = 0; i < 6; i++) { L.cols[i] = cols[i]; L.img[i] = img[i]; L.img_k[i] = img_k[i]; L.off[i + 1] = L.off[i] + rows[i] * (cols[i] ? cols[i] : 1); }
    } else {
        d.h1 = d.h2 = 0; d.n1 = d.n2 = 0;
        d.o_w1 = d.o_b1 = d.o_w2 = d.o_b2 = 0; d.o_w3 = 0; d.o_b3 = d.n3 * d.k1;   // (the bias block stays zero: ev2g_ac_tile adds it)
        d.stride = (long long)d.o_b3 + d.n3;
        L.n_arrays = 1; L.cols[0] = d_in; L.img[0] = 0; L.img_k[0] = d.k1; L.off[1] = d_out * d_in;
        for (int i = 1; i < EV2G_ARS_ARRAYS; i++) L.off[i + 1] = L.off[1];
    }
    L.n_params = L.off[L.n_arrays];
    p.lds = ev2g_ars_lds(d).bytes;
    p.image_bytes = (size_t)(1 + 2 * (long long)n_delta) * (size_t)d.stride * sizeof(float);
    p.delta_bytes = (size_t)n_delta * (size_t)L.n_params * sizeof(float);
    p.state_bytes = (size_t)L.n_params * sizeof(float) + (size_t)2 * n_delta * sizeof(double) + (size_t)2 * n_delta * sizeof(int32_t) + sizeof(ev2g_ars_report);
    p.total_bytes = p.image_bytes + p.delta_bytes + p.state_bytes;
    return p;
}

// ---- element functions shared by the kernels and the host twins ----
// candidates k and n_delta + k of one element: d = delta * (float)delta_std, theta +- d, each a float32 operation rounded once
__host__ __device__ inline void ars_perturb_elem(float theta, float delta, float std32, float *plus, float *minus) {
    const float d = delta * std32;
    *plus = theta + d; *minus = theta - d;
}
// the draw index of direction k's element i of iteration n: delta = ev2g_ac_normal(seed, index), the counter-based generator of ev2g_ac.h
__host__ __device__ inline uint64_t ars_delta_index(uint64_t n, int n_delta, int n_params, int k, int i) {
    return (n * (uint64_t)n_delta + (uint64_t)k) * (uint64_t)n_params + (uint64_t)i;
}
// env e's running return over the kept reward rows [k, stride], t ascending, on top of what it holds
__host__ __device__ inline double ars_env_return(double acc, const double *reward, int k, long long stride, long long e) {
    for (int t = 0; t < k; t++) acc += reward[(long long)t * stride + e];
    return acc;
}
// candidate c's return: its R envs ascending, then the alive bonus of the steps they took
__host__ __device__ inline double ars_candidate_return(const double *env_return, int R, int c, double alive_bonus_offset, long long steps) {
    double s = 0.0;
    for (int e = 0; e < R; e++) s += env_return[(long long)c * R + e];
    return s + alive_bonus_offset * (double)((long long)R * steps);
}
__host__ __device__ inline double ars_score(const double *ret, int n_delta, int k) { return ret[k] > ret[n_delta + k] ? ret[k] : ret[n_delta + k]; }
// direction k's rank: how many directions score higher, or the same with a lower index
__host__ __device__ inline int ars_rank_of(const double *ret, int n_delta, int k) {
    const double s = ars_score(ret, n_delta, k);
    int r = 0;
    for (int j = 0; j < n_delta; j++) {
        const double sj = ars_score(ret, n_delta, j);
        r += (sj > s || (sj == s && j < k)) ? 1 : 0;
    }
    return r;
}
__host__ __device__ inline bool ars_finite(double v) { return v - v == 0.0; }
// the first candidate whose return is not finite, or -1
__host__ __device__ inline int ars_first_bad(const double *ret, int n_delta) {
    for (int c = 0; c < 2 * n_delta; c++)
        if (!ars_finite(ret[c])) return c;
    return -1;
}
// sigma_R and the step from the kept directions (order[r]: the direction of rank r), serially
__host__ __device__ inline void ars_step_of(const double *ret, const int32_t *order, int n_delta, int n_top, double lr, double *sigma, double *step) {
    double sum = 0.0;
    for (int h = 0; h < 2; h++)
        for (int r = 0; r < n_top; r++) sum += ret[h * n_delta + order[r]];
    const double mean = sum / (double)(2 * n_top);
    double sq = 0.0;
    for (int h = 0; h < 2; h++)
        for (int r = 0; r < n_top; r++) { const double d = ret[h * n_delta + order[r]] - mean; sq += d * d; }
    *sigma = sqrt(sq / (double)(2 * n_top - 1));
    *step = lr / ((double)n_top * *sigma + 1e-6);
}
// theta_i after the step
__host__ __device__ inline float ars_theta_elem(float theta, const double *ret, const int32_t *order, const float *delta, int n_delta, int n_top, int n_params,
                                                int i, double step) {
    double acc = 0.0;
    for (int r = 0; r < n_top; r++) {
        const int k = order[r];
        acc += (ret[k] - ret[n_delta + k]) * (double)delta[(long long)k * n_params + i];
    }
    return (float)((double)theta + step * acc);
}

// ---- host twins ----
// delta [n_delta, n_params] of iteration n, and the 2 n_delta candidates' parameter vectors cand [2 n_delta, n_params] (may be null).  `normal`:
// float(uint64_t seed, uint64_t index), the library passes ev2g_ac_normal (which needs the device headers; this header does not)
template <class Normal>
inline void ars_host_perturb(const float *theta, int n_delta, int n_params, double delta_std, uint64_t seed, uint64_t n, float *delta, float *cand, Normal normal) {
    const float s = (float)delta_std;
    for (int k = 0; k < n_delta; k++)
        for (int i = 0; i < n_params; i++) {
            const float d = normal(seed, ars_delta_index(n, n_delta, n_params, k, i));
            delta[(long long)k * n_params + i] = d;
            if (cand) ars_perturb_elem(theta[i], d, s, cand + (long long)k * n_params + i, cand + (long long)(n_delta + k) * n_params + i);
        }
}
// env_return [E] += the kept rows reward [k, stride] (null or k 0: nothing), t ascending per env; returns [C] (may be null) of C candidates of E / C envs
inline void ars_host_returns(double *env_return, const double *reward, int k, long long stride, long long E, int C, double alive_bonus_offset, long long steps,
                             double *returns) {
    if (reward)
        for (long long e = 0; e < E; e++) env_return[e] = ars_env_return(env_return[e], reward, k, stride, e);
    if (returns)
        for (int c = 0; c < C; c++) returns[c] = ars_candidate_return(env_return, (int)(E / C), c, alive_bonus_offset, steps);
}
// the update on returns [2 n_delta]: theta in place, rank [n_delta] (direction k's rank), the report's figures
inline void ars_host_update(float *theta, const float *delta, const double *returns, int n_delta, int n_top, int n_params, double lr, int32_t *rank,
                            ev2g_ars_report *rep) {
    std::vector<int32_t> order((size_t)n_delta);
    for (int k = 0; k < n_delta; k++) { rank[k] = ars_rank_of(returns, n_delta, k); order[(size_t)rank[k]] = k; }
    rep->first_bad = ars_first_bad(returns, n_delta);
    rep->refused = rep->first_bad >= 0 ? 1 : 0;
    rep->n_top = n_top;
    rep->sigma_r = 0.0; rep->step = 0.0;
    if (rep->refused) return;
    ars_step_of(returns, order.data(), n_delta, n_top, lr, &rep->sigma_r, &rep->step);
    for (int i = 0; i < n_params; i++) theta[i] = ars_theta_elem(theta[i], returns, order.data(), delta, n_delta, n_top, n_params, i, rep->step);
}
// a parameter vector into / out of a candidate's image (padding untouched)
inline void ars_pack(const ArsLayout &L, const float *theta, float *image) {
    for (int i = 0; i < L.n_params; i++) image[ars_image_index(L, i)] = theta[i];
}
inline void ars_unpack(const ArsLayout &L, const float *image, float *theta) {
    for (int i = 0; i < L.n_params; i++) theta[i] = image[ars_image_index(L, i)];
}
