// ev2g_td3.h -- the off-policy learner of the device replay ring: SB3's TD3.train() for TD3Policy on a Box action space, one gradient step per
// call, with DDPG as the preset n_critics 1 / policy_delay 1 / no target noise; and ev2g_replay_sample, the uniform sampler of the ring.
//
// Per step on a batch (s, a, r, s', done) of B rows, update counter n incremented first:
//     eps = clamp(sigma * N(0, 1), -c, +c);  a' = clamp(actor_target(s') + eps, -1, 1);  y = r + ((1 - done) * gamma) * min_j critic_target_j(s', a')
//     critic_loss = sum_j mean((critic_j(s, a~) - y)^2)  -> Adam over every critic's parameters
//     n % policy_delay == 0:  actor_loss = -mean(critic_0(s, actor(s))) with critic_0 AFTER its step -> Adam on the actor, then
//                             target <- (1 - tau) * target + tau * param for the critics and the actor
// ACTIONS: the replay ring stores the env's action in the box [lo, 1]; the critics take SB3's scaled action in [-1, 1].  With lo = -1 the two are
// the same number; with lo = 0 the learner reads a~ = 2 a - 1.  actor(s) is the tanh output itself (the policy object's launches unscale it to
// [lo, 1] when they write an env action).  `done` is used as stored (the reference registers no time limit: episode ends are terminal).
//
// WHY LAYER-WISE: PPO's gradient kernel keeps a 256-wide network's activations and deltas of 32 rows in LDS.  A 400-300 actor with two critics
// keeps about 1 700 floats per row: 32 rows exceed 200 KB, more than a CU's 160 KB.  Here every layer is one launch over a learner-owned
// global workspace, and the twin critics (and their targets) are the z dimension of the same launch.
//
// One product kernel serves the forward layer, the backward-data layer and the weight gradient: C[m, n] = sum_k A(m, k) Bm(k, n) with strided
// operands, 16 x 16 tiles staged through LDS, and ONE fused-multiply-add chain per output element that runs k ascending from 0: float32 for the
// layers (k: a layer's width), float64 rounded once for the weight gradient (k: the batch row, rows ascending, no slab reduction -- a float32
// chain over 1024 rows drifts by about sqrt(1024) roundings, ten float32 ulps of the array's largest element where torch's float32 keeps one;
// a float32 product is exact in float64).  Bias gradients are float64 column sums and the losses float64 sums,
// each in one fixed order of rows (strided partials, rows ascending within one, joined in lane order) and rounded once.  No atomics, no kernel waits on another workgroup: the same call on the same state gives the same bits.  Masters are
// float32 in SB3's [out, in] layout; the bound policy object's packed images are rewritten from the actor's masters after every actor step,
// element by element through mlp_image_map (ev2g_policy_host.h), padding untouched.
#pragma once
#include <stdint.h>
#include <math.h>

// ---- element functions shared with the host twins (a host program defines __host__ and __device__ to nothing) ----
// SB3's polyak_update: target.mul_(1 - tau); target.add_(param, alpha = tau).  omt is 1 - tau rounded from float64.
__host__ __device__ inline float ev2g_polyak_elem(float target, float param, float omt, float tau) { return target * omt + tau * param; }
// target policy smoothing of one element: `normal` is the standard normal of its draw, sigma = 0 draws nothing (normal is not read)
__host__ __device__ inline float ev2g_td3_smooth_elem(float a_target, float normal, float sigma, float clip) {
    float eps = 0.0f;
    if (sigma > 0.0f) { eps = sigma * normal; eps = eps < -clip ? -clip : (eps > clip ? clip : eps); }
    const float a = a_target + eps;
    return a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a);
}
// y of one row: q_min is the smallest target critic's value
__host__ __device__ inline float ev2g_td3_y_elem(float r, uint8_t done, float gamma, float q_min) { return r + ((1.0f - (float)done) * gamma) * q_min; }
// the stored env action as the critic reads it
__host__ __device__ inline float ev2g_td3_scale_action(float a, float lo) { return lo == 0.0f ? 2.0f * a - 1.0f : a; }
// the sampler: row `row` of draw `counter` reads uniforms 3 i, 3 i + 1, 3 i + 2 of ev2g_host_uniform's generator under the seed, i = counter *
// EV2G_TD3_MAX_BATCH + row, and picks (entry of the complete list, step, env) as floor(u * n) clamped to n - 1
__host__ __device__ inline uint64_t ev2g_replay_stream_index(uint64_t counter, int row) { return (counter * 1024ull + (uint64_t)row) * 3ull; }
__host__ __device__ inline int ev2g_replay_pick(double u, int n) { const int i = (int)(u * (double)n); return i < n - 1 ? i : n - 1; }

// one bf16 term of a weight: the round-to-nearest-even bf16 of *r (host_bf16's bits), which *r then no longer holds (the subtraction is exact)
__host__ __device__ inline uint16_t ev2g_bf16_term(float *r) {
    uint32_t u;
    __builtin_memcpy(&u, r, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    const uint16_t hb = (uint16_t)(u >> 16);
    const uint32_t w = (uint32_t)hb << 16;
    float hf;
    __builtin_memcpy(&hf, &w, 4);
    *r -= hf;
    return hb;
}

#ifdef __HIPCC__
#define EV2G_TD3_TILE 16
enum { TD3_EPI_NONE = 0, TD3_EPI_BIAS, TD3_EPI_BIAS_RELU, TD3_EPI_BIAS_TANH, TD3_EPI_MASK };
// C[z][m, n] = epilogue(sum_k A[z](m, k) * Bm[z](k, n)); element (m, k) of A at A + z zA + m sam + k sak, (k, n) of Bm at Bm + z zB + k sbk + n sbn,
// C row stride ldc.  BIAS*: + bias[z][n] then the activation.  MASK: 0 where H[z][m, n] <= 0 (ReLU's derivative from its output; H row stride ldh).
// acc64: the chain runs in float64 and is rounded to float32 once, ahead of the epilogue (the weight gradient).
struct Td3Gemm {
    const float *A, *Bm, *bias, *H;
    float *C;
    int M, N, K, sam, sak, sbk, sbn, ldc, ldh, epi, acc64;
    long long zA, zB, zbias, zH, zC;
};
__global__ void __launch_bounds__(EV2G_TD3_TILE *EV2G_TD3_TILE) ev2g_td3_gemm_kernel(const Td3Gemm g) {
    __shared__ float As[EV2G_TD3_TILE][EV2G_TD3_TILE + 1], Bs[EV2G_TD3_TILE][EV2G_TD3_TILE + 1];
    const int tx = threadIdx.x, ty = threadIdx.y, z = blockIdx.z;
    const int m = blockIdx.y * EV2G_TD3_TILE + ty, n = blockIdx.x * EV2G_TD3_TILE + tx;
    const float *A = g.A + (long long)z * g.zA, *Bm = g.Bm + (long long)z * g.zB;
    float acc = 0.0f;
    double acc_d = 0.0;
    for (int k0 = 0; k0 < g.K; k0 += EV2G_TD3_TILE) {
        const int ka = k0 + tx, kb = k0 + ty;
        As[ty][tx] = (m < g.M && ka < g.K) ? A[(long long)m * g.sam + (long long)ka * g.sak] : 0.0f;
        Bs[ty][tx] = (kb < g.K && n < g.N) ? Bm[(long long)kb * g.sbk + (long long)n * g.sbn] : 0.0f;
        __syncthreads();
        const int kn = g.K - k0 < EV2G_TD3_TILE ? g.K - k0 : EV2G_TD3_TILE;   // (a padded product would be + 0 * 0: the same bits, skipped)
        if (g.acc64)
            for (int k = 0; k < kn; k++) acc_d = fma((double)As[ty][k], (double)Bs[k][tx], acc_d);
        else
            for (int k = 0; k < kn; k++) acc = fmaf(As[ty][k], Bs[k][tx], acc);
        __syncthreads();
    }
    if (g.acc64) acc = (float)acc_d;
    if (m >= g.M || n >= g.N) return;
    if (g.epi == TD3_EPI_BIAS || g.epi == TD3_EPI_BIAS_RELU || g.epi == TD3_EPI_BIAS_TANH) {
        acc += g.bias[(long long)z * g.zbias + n];
        if (g.epi == TD3_EPI_BIAS_RELU) acc = acc > 0.0f ? acc : 0.0f;
        if (g.epi == TD3_EPI_BIAS_TANH) acc = tanhf(acc);
    } else if (g.epi == TD3_EPI_MASK) {
        if (!(g.H[(long long)z * g.zH + (long long)m * g.ldh + n] > 0.0f)) acc = 0.0f;
    }
    g.C[(long long)z * g.zC + (long long)m * g.ldc + n] = acc;
}

// out[z][n] = sum over the rows of X[z][b, n], in float64, rounded once: 16 columns x 16 row lanes per workgroup; lane r adds rows r, r + 16, ...
// ascending, then the column's 16 partials are added in lane order.  One fixed order whatever the launch.
__global__ void __launch_bounds__(256) ev2g_td3_colsum_kernel(const float *__restrict__ X, long long zX, int B, int N, float *__restrict__ out, long long zout) {
    __shared__ double part[16][17];
    const int c = threadIdx.x & 15, r = threadIdx.x >> 4, n = blockIdx.x * 16 + c, z = blockIdx.y;
    const float *x = X + (long long)z * zX;
    double s = 0.0;
    if (n < N)
        for (int b = r; b < B; b += 16) s += (double)x[(long long)b * N + n];
    part[r][c] = s;
    __syncthreads();
    if (r == 0 && n < N) {
        double t = part[0][c];
        for (int i = 1; i < 16; i++) t += part[i][c];
        out[(long long)z * zout + n] = (float)t;
    }
}

// sum over i < n of f(i) in float64 by one workgroup of 256: thread t adds i = t, t + 256, ... ascending, thread 0 adds the partials in thread order
template <class F>
__device__ __forceinline__ double ev2g_td3_block_sum(int n, double *red, F f) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += f(i);
    red[threadIdx.x] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < 256; i++) t += red[i];
    __syncthreads();
    return t;   // (thread 0's)
}

// dst[b, 0 .. D) = obs[b, :];  dst[b, D + p] = scale(actions[b, p]) (actions null: the action columns are left alone)
__global__ void ev2g_td3_concat_kernel(const float *__restrict__ obs, const float *__restrict__ actions, int B, int D, int P, float lo, float *__restrict__ dst) {
    const int DA = D + P;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (long long)B * DA; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / DA), c = (int)(i % DA);
        if (c < D) dst[i] = obs[(long long)b * D + c];
        else if (actions) dst[i] = ev2g_td3_scale_action(actions[(long long)b * P + (c - D)], lo);
    }
}

// the action columns of dst [B, D + P] from act [B, P]: smoothed (SMOOTH: the target policy's noise, draw index first_draw + b P + p) or copied
template <bool SMOOTH>
__global__ void ev2g_td3_action_cols_kernel(const float *__restrict__ act, int B, int D, int P, float sigma, float clip, uint64_t seed, uint64_t first_draw,
                                            float *__restrict__ dst) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (long long)B * P; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / P), p = (int)(i % P);
        float a = act[i];
        if (SMOOTH) a = ev2g_td3_smooth_elem(a, sigma > 0.0f ? ev2g_ac_normal(seed, first_draw + (uint64_t)i) : 0.0f, sigma, clip);
        dst[(long long)b * (D + P) + D + p] = a;
    }
}

// y [B] from the target critics' values tq [nc, B]; then dq [nc, B] = 2 (q - y) / B and losses[0] = sum_j mean((q_j - y)^2).  One workgroup.
__global__ void __launch_bounds__(256) ev2g_td3_critic_head_kernel(const float *__restrict__ tq, const float *__restrict__ q, const float *__restrict__ reward,
                                                                   const uint8_t *__restrict__ done, int B, int nc, float gamma, float *__restrict__ y,
                                                                   float *__restrict__ dq, float *__restrict__ losses) {
    const double inv_b = 1.0 / (double)B;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float qm = tq[b];
        for (int j = 1; j < nc; j++) qm = fminf(qm, tq[(long long)j * B + b]);
        const float yb = ev2g_td3_y_elem(reward[b], done[b], gamma, qm);
        y[b] = yb;
        for (int j = 0; j < nc; j++) dq[(long long)j * B + b] = (float)(2.0 * ((double)q[(long long)j * B + b] - (double)yb) * inv_b);
    }
    __syncthreads();
    __shared__ double red[256];
    double total = 0.0;
    for (int j = 0; j < nc; j++)
        total += ev2g_td3_block_sum(B, red, [&](int b) { const double d = (double)q[(long long)j * B + b] - (double)y[b]; return d * d; }) * inv_b;
    if (threadIdx.x == 0) losses[0] = (float)total;
}

// the actor's head: dq [B] = -1 / B and losses[1] = -mean(q)
__global__ void __launch_bounds__(256) ev2g_td3_actor_head_kernel(const float *__restrict__ q, int B, float *__restrict__ dq, float *__restrict__ losses) {
    const double inv_b = 1.0 / (double)B;
    for (int b = threadIdx.x; b < B; b += blockDim.x) dq[b] = (float)(-inv_b);
    __shared__ double red[256];
    const double s = ev2g_td3_block_sum(B, red, [&](int b) { return (double)q[b]; });
    if (threadIdx.x == 0) losses[1] = (float)(-s * inv_b);
}

// d [i] *= 1 - t[i]^2: through the tanh of the actor's output
__global__ void ev2g_td3_tanh_back_kernel(float *__restrict__ d, const float *__restrict__ t, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) d[i] = d[i] * (1.0f - t[i] * t[i]);
}

__global__ void ev2g_td3_adam_kernel(float *__restrict__ theta, float *__restrict__ m, float *__restrict__ v, const float *__restrict__ grad, long long n,
                                     const AdamStep a) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        ev2g_adam_elem(theta + i, m + i, v + i, grad[i], a);
}

__global__ void ev2g_td3_polyak_kernel(float *__restrict__ target, const float *__restrict__ theta, long long n, float omt, float tau) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        target[i] = ev2g_polyak_elem(target[i], theta[i], omt, tau);
}

// The bound policy's images from the actor's masters (theta: W1 | b1 | W2 | b2 | W3 | b3 in SB3's layout), element by element through the map.
__global__ void ev2g_td3_refresh_kernel(const MlpImageMap mp, const float *__restrict__ theta) {
    for (int l = 0; l < 3; l++) {
        const MlpLayerMap &L = mp.layer[l];
        const float *W = theta + L.w_off, *b = theta + L.b_off;
        for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (long long)L.n_out * L.n_in; i += (long long)gridDim.x * blockDim.x) {
            const int n = (int)(i / L.n_in), k = (int)(i % L.n_in);
            if (L.kind == MLP_IMG_F32) ((float *)L.w)[mlp_image_index(L, n, k, 0)] = W[i];
            else {
                float r = W[i];
                for (int q = 0; q < L.nw; q++) {
                    const uint16_t hb = ev2g_bf16_term(&r);
                    ((uint16_t *)L.w)[mlp_image_index(L, n, k, q)] = hb;
                }
            }
        }
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n_out; i += gridDim.x * blockDim.x) L.bias[i] = b[i];
    }
}

// ---- the sampler of a replay ring ----
#define EV2G_REPLAY_MAX_BLOCKS 32
struct ReplayTable {
    const float *obs[EV2G_REPLAY_MAX_BLOCKS], *actions[EV2G_REPLAY_MAX_BLOCKS];
    const double *reward[EV2G_REPLAY_MAX_BLOCKS];
    const uint8_t *done[EV2G_REPLAY_MAX_BLOCKS];
    int n, T, E, D, P;   // n: complete blocks listed (the table holds only those, in the list's order)
};
// one workgroup per batch row: thread 0 draws (block, t, e), all threads copy the row's columns
__global__ void __launch_bounds__(64) ev2g_replay_sample_kernel(const ReplayTable tb, uint64_t seed, uint64_t counter, float *__restrict__ obs,
                                                                float *__restrict__ actions, float *__restrict__ reward, float *__restrict__ next_obs,
                                                                uint8_t *__restrict__ done, int *__restrict__ index) {
    const int row = blockIdx.x;
    const uint64_t i0 = ev2g_replay_stream_index(counter, row);
    const int bi = ev2g_replay_pick(ev2g_u01(seed, i0), tb.n), t = ev2g_replay_pick(ev2g_u01(seed, i0 + 1), tb.T), e = ev2g_replay_pick(ev2g_u01(seed, i0 + 2), tb.E);
    const float *so = tb.obs[bi] + ((long long)t * tb.E + e) * tb.D, *sn = so + (long long)tb.E * tb.D;
    const float *sa = tb.actions[bi] + ((long long)t * tb.E + e) * tb.P;
    for (int c = threadIdx.x; c < tb.D; c += blockDim.x) { obs[(long long)row * tb.D + c] = so[c]; next_obs[(long long)row * tb.D + c] = sn[c]; }
    for (int c = threadIdx.x; c < tb.P; c += blockDim.x) actions[(long long)row * tb.P + c] = sa[c];
    if (threadIdx.x == 0) {
        reward[row] = (float)tb.reward[bi][(long long)t * tb.E + e];
        done[row] = tb.done[bi][(long long)t * tb.E + e];
        if (index) { index[3 * row] = bi; index[3 * row + 1] = t; index[3 * row + 2] = e; }
    }
}
#endif
