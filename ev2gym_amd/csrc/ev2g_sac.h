// ev2g_sac.h -- SB3's SAC.train() for SACPolicy (MlpPolicy, Box actions, use_sde off) on the device, one gradient step per call, and the
// stochastic actor its collector runs.
//
//   actor    h = ReLU(W2 ReLU(W1 s + b1) + b2);  mu = Wmu h + bmu;  log_std = clamp(Wls h + bls, -20, 2);  u = mu + exp(log_std) eps;  a = tanh(u)
//            log pi = sum_p [ -eps^2 / 2 - log_std - log(2 pi) / 2 ] - sum_p log(1 - a^2 + 1e-6)
//   critics  n_critics of (s, a) -> h1 -> h2 -> 1 with ReLU, and their targets (no actor target)
//
// The Gaussian term is the reduced form of Normal(mu, sigma).log_prob(mu + sigma eps): the literal form cancels (mu + sigma eps) - mu, which
// loses every digit once sigma = e^-20.  Per update on (s, a~, r, s', done) of B rows, alpha = exp(log_ent_coef) as it stands before the update
// and d the learner's draw base:
//     eps  = draws d + b P + p:          a_pi, log pi on s;        d loss / d log alpha = -mean(log pi + target_entropy)
//     eps' = draws d + B P + b P + p:    a', log pi' on s';        y = r + ((1 - done) gamma) (min_j target_j(s', a') - alpha log pi')
//     critic_loss = 0.5 sum_j mean((Q_j(s, a~) - y)^2)  -> Adam on all critics
//     actor_loss = mean(alpha log pi - min_j Q_j(s, a_pi)) with the critics AFTER their step, through each row's argmin critic -> Adam on the actor
//     Adam on log alpha (not for a fixed coefficient); every target_update_interval-th update target <- (1 - tau) target + tau param (critics)
//     d += 2 B P; the collection actor's packed images are rewritten from the masters
//
// LAYER-WISE like ev2g_td3.h, and through its kernels: the product kernel, the column sums, concat, Adam and Polyak.  The mu and log_std heads
// are the z dimension of one launch (Wmu | bmu and Wls | bls are two blocks of one size in SB3's parameter order); their two backward-data
// products meet in ev2g_sac_join_kernel.  With two critics dQ_min / da is the sum of both critics' input deltas, where the critic that is not
// a row's argmin was given an output delta of exactly 0.  The heads (B P elements) are float64 from the stored float32 mu, raw log_std and
// eps, every output rounded once; sums run in one fixed order; no atomics: the same call on the same state gives the same bits.
//
// THE COLLECTION ACTOR (ev2g_sac_act_kernel) is ev2g_ac.h's 32-row exact-f32 MFMA tile over pack_linear_f32 images: ReLU trunk, then the two
// heads as linear tiles of ONE stacked image (head i's rows start at i * n3, a 32-column boundary), then eight lanes per row draw eps,
// squash and unscale.  A row's outputs are one fixed k-ordered chain of that row.  Draw (n E + e) P + p for the object's n-th sampling
// launch, under a seed and counter of the collection stream's own.
#pragma once
#include <stdint.h>
#include <math.h>

#define EV2G_SAC_LOG_STD_MIN (-20.0)
#define EV2G_SAC_LOG_STD_MAX 2.0
#define EV2G_SAC_EPS 1e-6
#define EV2G_SAC_HALF_LOG_2PI 0.9189385332046727

// ---- element functions shared with the host twins (a host program defines __host__ and __device__ to nothing) ----
// one element of the squashed-Gaussian head in float64: the tanh action and the element's term of log pi
__host__ __device__ inline void ev2g_sac_head_elem(float mu, float log_std_raw, float eps, double *a, double *lp) {
    double ls = (double)log_std_raw;
    ls = ls < EV2G_SAC_LOG_STD_MIN ? EV2G_SAC_LOG_STD_MIN : (ls > EV2G_SAC_LOG_STD_MAX ? EV2G_SAC_LOG_STD_MAX : ls);
    const double e = (double)eps, t = tanh((double)mu + exp(ls) * e);
    *a = t;
    *lp = ((-0.5 * e * e - ls) - EV2G_SAC_HALF_LOG_2PI) - log((1.0 - t * t) + EV2G_SAC_EPS);
}
// ... and its backward: g = dQ_min / da of the element, inv_b = 1 / B
__host__ __device__ inline void ev2g_sac_head_back_elem(float mu, float log_std_raw, float eps, double g, double alpha, double inv_b, double *d_mu,
                                                        double *d_log_std) {
    const double raw = (double)log_std_raw;
    const double ls = raw < EV2G_SAC_LOG_STD_MIN ? EV2G_SAC_LOG_STD_MIN : (raw > EV2G_SAC_LOG_STD_MAX ? EV2G_SAC_LOG_STD_MAX : raw);
    const double e = (double)eps, sigma = exp(ls), t = tanh((double)mu + sigma * e), omt = 1.0 - t * t;
    const double du = (alpha * (2.0 * t * omt / (omt + EV2G_SAC_EPS)) - g * omt) * inv_b;
    *d_mu = du;
    *d_log_std = (raw > EV2G_SAC_LOG_STD_MIN && raw < EV2G_SAC_LOG_STD_MAX) ? du * sigma * e - alpha * inv_b : 0.0;
}
// y of one row: q_min the smallest target critic's value on (s', a'), lp the log pi of a'
__host__ __device__ inline float ev2g_sac_y_elem(float r, uint8_t done, double gamma, float q_min, double alpha, float lp) {
    return (float)((double)r + ((1.0 - (double)done) * gamma) * ((double)q_min - alpha * (double)lp));
}
// the tanh action as the env takes it, in the box [lo, 1] (the inverse of ev2g_td3_scale_action)
__host__ __device__ inline float ev2g_sac_unscale_action(float a, float lo) { return lo == 0.0f ? 0.5f * (a + 1.0f) : a; }
__host__ __device__ inline double ev2g_sac_alpha(float log_alpha) { return exp((double)log_alpha); }

// the collection actor's network: the widths, the padded widths (inputs to 8, columns to 32) and the images
struct SacDev {
    int d_in, h1, h2, d_out;
    int k1, n1, n2, n3;
    float lo;
    float *w1, *b1, *w2, *b2;   // trunk: pack_linear_f32 images, biases padded with zeros
    float *wh, *bh;             // the stacked heads: [2 n3, n2] packed, [2 n3]
};
struct SacLds { int sA, sB; size_t bytes; };
// two activation blocks of 32 rows (float32, +16 bytes per row): A the input rows, then the second hidden layer; B the first, then mu | log_std
__host__ __device__ inline SacLds ev2g_sac_lds(const SacDev &m) {
    SacLds l;
    l.sA = (m.k1 > m.n2 ? m.k1 : m.n2) + 4; l.sB = (m.n1 > 2 * m.n3 ? m.n1 : 2 * m.n3) + 4;
    l.bytes = (size_t)32 * (l.sA + l.sB) * sizeof(float);
    return l;
}
// (the largest network of the limits, 192 -> 256 -> 256 -> 64: 66560 bytes)
inline size_t ev2g_sac_lds_max() { return (size_t)32 * 2 * (256 + 4) * sizeof(float); }

#ifdef __HIPCC__
// The head of B rows: eight lanes per row, lane j takes p = j, j + 8, ..., the eight partial sums of log pi meet in a fixed butterfly.  Writes
// eps, a [B, P], a into columns [col0, col0 + P) of xcols (row stride ldx; the critics' input) and log pi [B].
__global__ void __launch_bounds__(256) ev2g_sac_head_kernel(const float *__restrict__ mu, const float *__restrict__ ls, int B, int P, uint64_t seed, uint64_t draw0,
                                                            float *__restrict__ eps_out, float *__restrict__ a_out, float *__restrict__ xcols, int ldx, int col0,
                                                            float *__restrict__ logp) {
    const int row = blockIdx.x * 32 + (threadIdx.x >> 3), j = threadIdx.x & 7;
    const bool live = row < B;
    double lp = 0.0;
    if (live)
        for (int p = j; p < P; p += 8) {
            const long long i = (long long)row * P + p;
            const float e = ev2g_ac_normal(seed, draw0 + (uint64_t)i);
            double a, t;
            ev2g_sac_head_elem(mu[i], ls[i], e, &a, &t);
            lp += t;
            eps_out[i] = e; a_out[i] = (float)a;
            xcols[(long long)row * ldx + col0 + p] = (float)a;
        }
    lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 1);
    if (live && j == 0) logp[row] = (float)lp;
}

// d_mu, d_log_std [B, P] (d_head and d_head + B P) from g = sum_j dxa[j] [B, P]: the critics' input deltas, exactly 0 off a row's argmin
__global__ void ev2g_sac_head_back_kernel(const float *__restrict__ mu, const float *__restrict__ ls, const float *__restrict__ eps, const float *__restrict__ dxa,
                                          int nc, int B, int P, const float *__restrict__ log_alpha, float *__restrict__ d_head) {
    const double alpha = ev2g_sac_alpha(*log_alpha), inv_b = 1.0 / (double)B;
    const long long n = (long long)B * P;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        double g = (double)dxa[i];
        if (nc == 2) g += (double)dxa[n + i];
        double dm, dl;
        ev2g_sac_head_back_elem(mu[i], ls[i], eps[i], g, alpha, inv_b, &dm, &dl);
        d_head[i] = (float)dm; d_head[n + i] = (float)dl;
    }
}

// out = a + b where h > 0, else 0: the two heads' backward-data products through the second hidden layer's ReLU
__global__ void ev2g_sac_join_kernel(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ h, long long n, float *__restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = h[i] > 0.0f ? a[i] + b[i] : 0.0f;
}

// y [B] from the target critics' values tq [nc, B] and log pi' [B]; dq [nc, B] = (q - y) / B; losses[0] = 0.5 sum_j mean((q_j - y)^2).  One workgroup.
__global__ void __launch_bounds__(256) ev2g_sac_critic_head_kernel(const float *__restrict__ tq, const float *__restrict__ q, const float *__restrict__ lp,
                                                                   const float *__restrict__ reward, const uint8_t *__restrict__ done, int B, int nc, double gamma,
                                                                   const float *__restrict__ log_alpha, float *__restrict__ y, float *__restrict__ dq,
                                                                   float *__restrict__ losses) {
    const double inv_b = 1.0 / (double)B, alpha = ev2g_sac_alpha(*log_alpha);
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float qm = tq[b];
        for (int j = 1; j < nc; j++) qm = fminf(qm, tq[(long long)j * B + b]);
        const float yb = ev2g_sac_y_elem(reward[b], done[b], gamma, qm, alpha, lp[b]);
        y[b] = yb;
        for (int j = 0; j < nc; j++) dq[(long long)j * B + b] = (float)(((double)q[(long long)j * B + b] - (double)yb) * inv_b);
    }
    __syncthreads();
    __shared__ double red[256];
    double total = 0.0;
    for (int j = 0; j < nc; j++)
        total += ev2g_td3_block_sum(B, red, [&](int b) { const double d = (double)q[(long long)j * B + b] - (double)y[b]; return d * d; }) * inv_b;
    if (threadIdx.x == 0) losses[0] = (float)(0.5 * total);
}

// The actor's head on q [nc, B] = Q_j(s, a_pi) and log pi [B]: sel [nc, B] = 1 at each row's argmin critic (the first of equals), 0 elsewhere --
// the critics' output delta; losses[1] = actor_loss, [2] = ent_coef_loss, [3] = alpha; g_alpha = -mean(log pi + target_entropy) (fixed: 0)
__global__ void __launch_bounds__(256) ev2g_sac_actor_head_kernel(const float *__restrict__ q, const float *__restrict__ lp, int B, int nc,
                                                                  const float *__restrict__ log_alpha, double target_entropy, int auto_alpha,
                                                                  float *__restrict__ sel, float *__restrict__ losses, float *__restrict__ g_alpha) {
    const double inv_b = 1.0 / (double)B, la = (double)*log_alpha, alpha = ev2g_sac_alpha(*log_alpha);
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int j = (nc == 2 && q[B + b] < q[b]) ? 1 : 0;
        for (int c = 0; c < nc; c++) sel[(long long)c * B + b] = c == j ? 1.0f : 0.0f;
    }
    __shared__ double red[256];
    const double s1 = ev2g_td3_block_sum(B, red, [&](int b) {
        const float qm = (nc == 2 && q[B + b] < q[b]) ? q[B + b] : q[b];
        return alpha * (double)lp[b] - (double)qm;
    });
    const double s2 = ev2g_td3_block_sum(B, red, [&](int b) { return (double)lp[b] + target_entropy; });
    if (threadIdx.x == 0) {
        const double g = -(s2 * inv_b);
        losses[1] = (float)(s1 * inv_b);
        losses[2] = auto_alpha ? (float)(la * g) : 0.0f;
        losses[3] = (float)alpha;
        *g_alpha = auto_alpha ? (float)g : 0.0f;
    }
}

// Adam on the one element log alpha: st = {log alpha, m, v}
__global__ void ev2g_sac_alpha_adam_kernel(float *__restrict__ st, const float *__restrict__ g, const AdamStep a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ev2g_adam_elem(st, st + 1, st + 2, *g, a);
}

// The collection actor's images from the actor's masters (theta: W1 | b1 | W2 | b2 | Wmu | bmu | Wls | bls at off[0 .. 8]), element by element:
// padding is never written.
struct SacRepack { int off[9]; };
__global__ void ev2g_sac_repack_kernel(const SacDev m, const SacRepack r, const float *__restrict__ theta) {
    const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, nt = (long long)gridDim.x * blockDim.x;
    for (long long i = tid; i < (long long)m.h1 * m.d_in; i += nt) m.w1[packed_f32_index((int)(i / m.d_in), (int)(i % m.d_in), m.k1)] = theta[r.off[0] + i];
    for (long long i = tid; i < (long long)m.h2 * m.h1; i += nt) m.w2[packed_f32_index((int)(i / m.h1), (int)(i % m.h1), m.n1)] = theta[r.off[2] + i];
    for (int hd = 0; hd < 2; hd++) {
        for (long long i = tid; i < (long long)m.d_out * m.h2; i += nt)
            m.wh[sac_head_index(hd, (int)(i / m.h2), (int)(i % m.h2), m.n3, m.n2)] = theta[r.off[4 + 2 * hd] + i];
        for (long long i = tid; i < m.d_out; i += nt) m.bh[hd * m.n3 + i] = theta[r.off[5 + 2 * hd] + i];
    }
    for (long long i = tid; i < m.h1; i += nt) m.b1[i] = theta[r.off[1] + i];
    for (long long i = tid; i < m.h2; i += nt) m.b2[i] = theta[r.off[3] + i];
}

// n_rows observation rows x [n_rows, D] -> the env action row act [n_rows, P] in [lo, 1] and (each may be null) mu, raw log_std [n_rows, P],
// log pi [n_rows].  SAMPLE: eps of element (row, p) is draw (draw0 + row) P + p under `seed`; else eps = 0 (a = tanh(mu)) and nothing is drawn.
template <bool SAMPLE>
__global__ void __launch_bounds__(EV2G_AC_BLOCK) ev2g_sac_act_kernel(SacDev m, const float *__restrict__ x, int n_rows, uint64_t seed, uint64_t draw0,
                                                                    float *__restrict__ act, float *__restrict__ mu_out, float *__restrict__ ls_out,
                                                                    float *__restrict__ logp) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    const SacLds L = ev2g_sac_lds(m);
    float *bufA = sac_lds, *bufB = bufA + EV2G_AC_ROWS * L.sA;
    const int wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * EV2G_AC_ROWS;
    const int nr = (int)(n_rows - row0 < EV2G_AC_ROWS ? n_rows - row0 : EV2G_AC_ROWS);
    // input rows -> LDS, zeros past the last row and past D
    for (int i = threadIdx.x; i < EV2G_AC_ROWS * m.k1; i += EV2G_AC_BLOCK) {
        const int r = i / m.k1, c = i - r * m.k1;
        bufA[r * L.sA + c] = (r < nr && c < m.d_in) ? x[(size_t)(row0 + r) * m.d_in + c] : 0.0f;
    }
    __syncthreads();
    {   // A -> B
        const int KG = m.k1 >> 3;
        for (int t = wave; t < (m.n1 >> 5); t += EV2G_AC_BLOCK / 64) ev2g_ac_tile<EV2G_AC_RELU>(bufA, L.sA, KG, m.w1 + (size_t)t * KG * 256, m.b1, t * 32, bufB, L.sB);
    }
    __syncthreads();
    {   // B -> A
        const int KG = m.n1 >> 3;
        for (int t = wave; t < (m.n2 >> 5); t += EV2G_AC_BLOCK / 64) ev2g_ac_tile<EV2G_AC_RELU>(bufB, L.sB, KG, m.w2 + (size_t)t * KG * 256, m.b2, t * 32, bufA, L.sA);
    }
    __syncthreads();
    {   // the stacked heads: A -> B (mu at column 0, raw log_std at column n3), linear
        const int KG = m.n2 >> 3;
        for (int t = wave; t < (2 * m.n3 >> 5); t += EV2G_AC_BLOCK / 64) ev2g_ac_tile<EV2G_AC_LINEAR>(bufA, L.sA, KG, m.wh + (size_t)t * KG * 256, m.bh, t * 32, bufB, L.sB);
    }
    __syncthreads();
    const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
    const bool live = row < nr;
    const long long grow = row0 + row;
    double lp = 0.0;
    if (live)
        for (int p = j; p < m.d_out; p += 8) {
            const float mu = bufB[row * L.sB + p], ls = bufB[row * L.sB + m.n3 + p];
            const float e = SAMPLE ? ev2g_ac_normal(seed, (draw0 + (uint64_t)grow) * (uint64_t)m.d_out + (uint64_t)p) : 0.0f;
            double a, t;
            ev2g_sac_head_elem(mu, ls, e, &a, &t);
            lp += t;
            const size_t o = (size_t)grow * m.d_out + p;
            act[o] = ev2g_sac_unscale_action((float)a, m.lo);
            if (mu_out) mu_out[o] = mu;
            if (ls_out) ls_out[o] = ls;
        }
    lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 1);
    if (live && j == 0 && logp) logp[grow] = (float)lp;
}
#endif
