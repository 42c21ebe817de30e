// ev2g_ac.h -- the on-policy half of the reference's training script (train_stable_baselines.py:24: PPO by default, A2C, TRPO): SB3's default
// ActorCriticPolicy for a Box action space evaluated and SAMPLED on the device, and RolloutBuffer.compute_returns_and_advantage (GAE).
//
//   policy trunk  obs[D] -> act(h1) -> act(h2) -> linear(P) = mean          value trunk  obs[D] -> act(v1) -> act(v2) -> linear(1) = value
//   act = tanh (SB3's default) or ReLU for both trunks; log_std[P] does not depend on the state
//   a = mean + exp(log_std) * eps,  log_prob = sum_p [ -(a - mean)^2 / (2 sigma^2) - log_std - log(2 pi) / 2 ]  on the UNCLIPPED a (as SB3 does),
//   a_env = clip(a, lo, 1),  lo in {-1, 0}: the reference's two action boxes (ev2gym_env.py:226-231)
//
// LIMITS: D <= 192, every hidden width <= 256, P <= 64.  Anything else is refused at create (EV2G_ERR_ARG); there is no generic fallback.  That
// covers the shipped V2G_profit_max_loads (D 162, P 50) and PublicPST (D 63, P 20) shapes.
//
// Arithmetic: float32 operands on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32, the operand layout of ev2g_mlp32_layer: pack_linear_f32), float32
// accumulation, no bf16 split -- the networks are small (64-64 by default), the weight stream is not the cost.  One workgroup of four wavefronts
// evaluates 32 observation rows: the column tiles of BOTH trunks' layer are shared out over the wavefronts, activations stay in LDS.  The value
// head (one column) is a plain FMA chain, eight lanes per row and a fixed butterfly.  Rows past the end and columns past a layer's width are
// zeros (zero weights, zero bias, act(0) = 0), every output element is one fixed k-ordered chain of its own row: a row's results do not depend
// on which rows share the launch or where the row sits in it (tests/test_onpolicy_gpu.py holds that bit for bit).
// The log-probability is summed in float64 from the stored float32 action and mean and rounded once.
//
// Noise: no stored stream.  eps of draw index j is Box-Muller on the uniforms 2 j and 2 j + 1 of ev2g_u01(seed, .), evaluated with the
// generator's own log / cos (ev2g_gen.h: fixed sequences of IEEE operations), so host (ev2g_ac_host_normal) and device give the same bits.
// Element (row e, port p) of the object's n-th sampling launch over E rows draws index (n E + e) P + p.
#pragma once
#include "ev2g_policy_host.h"   // EV2G_AC_MAX_IN / _HIDDEN / _OUT: the limits plan_ac refuses by

#define EV2G_AC_ROWS 32
#define EV2G_AC_BLOCK 256
#define EV2G_AC_DEPTH 8   // weight groups in flight per tile

struct AcDev {
    int d_in, h1, h2, v1, v2, d_out;   // the network's own widths
    int k1, n1, n2, m1, m2, n3;        // padded: inputs to 8, every layer's columns to 32
    float lo;
    const float *w1, *b1, *w2, *b2, *w3, *b3;   // policy trunk and action head, weights packed by pack_linear_f32, biases padded with zeros
    const float *u1, *c1, *u2, *c2;             // value trunk, likewise
    const float *u3, *c3;                       // value head: the weight row [m2] padded with zeros, the bias [1]
    const float *sigma;                         // [P] exp(log_std), rounded once from float64
    const double *lp_a, *lp_c;                  // [P] 1 / (2 sigma^2) and -log_std - log(2 pi) / 2, float64
};

struct AcLds { int sA, sB, sV, sC; size_t bytes; };
// four activation blocks of 32 rows (float32, +16 bytes per row against bank conflicts): A input rows, then the policy trunk's second layer;
// B the policy trunk's first layer, then the mean; V / C the value trunk's first / second layer
__host__ __device__ inline AcLds ev2g_ac_lds(const AcDev &m) {
    AcLds l;
    l.sA = (m.k1 > m.n2 ? m.k1 : m.n2) + 4; l.sB = (m.n1 > m.n3 ? m.n1 : m.n3) + 4; l.sV = m.m1 + 4; l.sC = m.m2 + 4;
    l.bytes = (size_t)EV2G_AC_ROWS * (l.sA + l.sB + l.sV + l.sC) * sizeof(float);
    return l;
}

// (the largest network of the limits: 133120 bytes of the CU's 160 KiB)
inline size_t ev2g_ac_lds_max() { return (size_t)EV2G_AC_ROWS * 4 * (EV2G_AC_MAX_HIDDEN + 4) * sizeof(float); }

// standard normal of draw index j under `seed`: the one definition, host and device
__host__ __device__ inline float ev2g_ac_normal(uint64_t seed, uint64_t j) {
    const double u1 = ev2g_u01(seed, 2 * j), u2 = ev2g_u01(seed, 2 * j + 1);   // [0, 1): 1 - u1 is in (0, 1]
    return (float)(sqrt(-2.0 * ev2g_dlog(1.0 - u1)) * ev2g_dcos(6.283185307179586 * u2));
}

#define EV2G_AC_TANH 0
#define EV2G_AC_RELU 1
#define EV2G_AC_LINEAR 2
// one 32-column tile of a layer for the workgroup's 32 rows: out[row][col0 + c] = act(bias + sum_k A[row][k] W[col0 + c][k]), k ascending in
// groups of eight (MFMA j of group g takes k = 8 g + j from lanes 0..31 and k = 8 g + 4 + j from lanes 32..63)
template <int ACT>
__device__ __forceinline__ void ev2g_ac_tile(const float *__restrict__ A, int sa, int KG, const float *__restrict__ Wt, const float *__restrict__ bias,
                                             int col0, float *__restrict__ out, int so) {
    const int lane = threadIdx.x & 63;
    const float *arow = A + (lane & 31) * sa + 4 * (lane >> 5);
    const f32x4 *w = (const f32x4 *)Wt + lane;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // the tile's weights come through a ring of EV2G_AC_DEPTH registers loaded that many groups ahead (as ev2g_mlp32_layer does): the loop
    // would otherwise wait out one L2 round trip per group of eight k
    f32x4 ring[EV2G_AC_DEPTH];
#pragma unroll
    for (int u = 0; u < EV2G_AC_DEPTH; u++) ring[u] = w[(size_t)min(u, KG - 1) * 64];
    for (int g0 = 0; g0 < KG; g0 += EV2G_AC_DEPTH) {
#pragma unroll
        for (int u = 0; u < EV2G_AC_DEPTH; u++) {
            const int g = g0 + u;
            if (g < KG) {   // (uniform)
                const f32x4 a = *(const f32x4 *)(arow + g * 8), b = ring[u];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
                ring[u] = w[(size_t)min(g + EV2G_AC_DEPTH, KG - 1) * 64];
            }
        }
    }
    const int col = col0 + (lane & 31);
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        float v = acc[r] + bv;
        if (ACT == EV2G_AC_TANH) v = tanhf(v);
        if (ACT == EV2G_AC_RELU) v = v > 0.0f ? v : 0.0f;
        out[row * so + col] = v;
    }
}

// Both trunks, both heads, the sample, its log-probability and the clip for n_rows observation rows x [n_rows, D].  Outputs (each may be null):
// mean / actions / clipped [n_rows, P], value / log_prob [n_rows].  sample != 0: a = mean + sigma eps with the draws (draw0 + row) P + p under
// `seed`; else a = mean.
template <int ACT>
__global__ void __launch_bounds__(EV2G_AC_BLOCK) ev2g_ac_act_kernel(AcDev m, const float *__restrict__ x, int n_rows, int sample, uint64_t seed,
                                                                   uint64_t draw0, float *__restrict__ mean, float *__restrict__ actions,
                                                                   float *__restrict__ clipped, float *__restrict__ value, float *__restrict__ log_prob) {
    extern __shared__ __attribute__((aligned(16))) float ac_lds[];
    const AcLds L = ev2g_ac_lds(m);
    float *bufA = ac_lds, *bufB = bufA + EV2G_AC_ROWS * L.sA, *bufV = bufB + EV2G_AC_ROWS * L.sB, *bufC = bufV + EV2G_AC_ROWS * L.sV;
    const int wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * EV2G_AC_ROWS;
    const int nr = (int)(n_rows - row0 < EV2G_AC_ROWS ? n_rows - row0 : EV2G_AC_ROWS);
    // input rows -> LDS, zeros past the last row and past D
    for (int i = threadIdx.x; i < EV2G_AC_ROWS * m.k1; i += EV2G_AC_BLOCK) {
        const int r = i / m.k1, c = i - r * m.k1;
        bufA[r * L.sA + c] = (r < nr && c < m.d_in) ? x[(size_t)(row0 + r) * m.d_in + c] : 0.0f;
    }
    __syncthreads();
    {   // first layers of both trunks: A -> B (policy), A -> V (value)
        const int KG = m.k1 >> 3, tp = m.n1 >> 5, tv = m.m1 >> 5;
        for (int t = wave; t < tp + tv; t += EV2G_AC_BLOCK / 64) {
            if (t < tp) ev2g_ac_tile<ACT>(bufA, L.sA, KG, m.w1 + (size_t)t * KG * 256, m.b1, t * 32, bufB, L.sB);
            else ev2g_ac_tile<ACT>(bufA, L.sA, KG, m.u1 + (size_t)(t - tp) * KG * 256, m.c1, (t - tp) * 32, bufV, L.sV);
        }
    }
    __syncthreads();
    {   // second layers: B -> A (policy), V -> C (value)
        const int KGp = m.n1 >> 3, KGv = m.m1 >> 3, tp = m.n2 >> 5, tv = m.m2 >> 5;
        for (int t = wave; t < tp + tv; t += EV2G_AC_BLOCK / 64) {
            if (t < tp) ev2g_ac_tile<ACT>(bufB, L.sB, KGp, m.w2 + (size_t)t * KGp * 256, m.b2, t * 32, bufA, L.sA);
            else ev2g_ac_tile<ACT>(bufV, L.sV, KGv, m.u2 + (size_t)(t - tp) * KGv * 256, m.c2, (t - tp) * 32, bufC, L.sC);
        }
    }
    __syncthreads();
    // eight lanes per row for the value head and the per-port epilogue: lane j takes k (p) = j, j + 8, ..., the eight partial sums meet in a
    // fixed butterfly
    const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
    float pv = 0.0f;
    for (int k = j; k < m.m2; k += 8) pv = fmaf(bufC[row * L.sC + k], m.u3[k], pv);
    pv += __shfl_xor(pv, 4); pv += __shfl_xor(pv, 2); pv += __shfl_xor(pv, 1);
    pv += m.c3[0];
    {   // action head: A -> B (the mean), linear
        const int KG = m.n2 >> 3, tp = m.n3 >> 5;
        for (int t = wave; t < tp; t += EV2G_AC_BLOCK / 64) ev2g_ac_tile<EV2G_AC_LINEAR>(bufA, L.sA, KG, m.w3 + (size_t)t * KG * 256, m.b3, t * 32, bufB, L.sB);
    }
    __syncthreads();
    const bool live = row < nr;
    const long long grow = row0 + row;
    double lp = 0.0;
    if (live) {
        for (int p = j; p < m.d_out; p += 8) {
            const float mu = bufB[row * L.sB + p];
            float a = mu;
            if (sample) a = mu + m.sigma[p] * ev2g_ac_normal(seed, (draw0 + (uint64_t)grow) * (uint64_t)m.d_out + (uint64_t)p);
            const double d = (double)a - (double)mu;
            lp += m.lp_c[p] - (d * d) * m.lp_a[p];
            const size_t o = (size_t)grow * m.d_out + p;
            if (mean) mean[o] = mu;
            if (actions) actions[o] = a;
            if (clipped) clipped[o] = fminf(fmaxf(a, m.lo), 1.0f);
        }
    }
    lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 1);
    if (live && j == 0) {
        if (value) value[grow] = pv;
        if (log_prob) log_prob[grow] = (float)lp;
    }
}

// ---- GAE: RolloutBuffer.compute_returns_and_advantage in float32, one env's backward walk; host (ev2g_host_gae) and device from this source ----
// g = (float)gamma, c = (float)(gamma * lambda) (the float64 product rounded once).  reward [k, E] float64 (the engine's), values [k, E],
// episode_starts [k, E] (row t: env e's step t is the first of an episode), last_values / last_dones [E]: the value of the observation behind
// the last row and whether that row ended an episode.
__host__ __device__ inline void ev2g_gae_env(const double *reward, const float *values, const uint8_t *episode_starts, const float *last_values,
                                             const uint8_t *last_dones, int k, long long E, long long e, float g, float c, float *advantages,
                                             float *returns) {
    float last = 0.0f;
    for (int t = k - 1; t >= 0; t--) {
        const long long i = (long long)t * E + e;
        const float next_start = t == k - 1 ? (float)last_dones[e] : (float)episode_starts[i + E];
        const float next_v = t == k - 1 ? last_values[e] : values[i + E];
        const float nnt = 1.0f - next_start;
        const float r = (float)reward[i], v = values[i];
        const float delta = (r + (g * next_v) * nnt) - v;
        const float adv = delta + (c * nnt) * last;
        advantages[i] = adv;
        returns[i] = adv + v;
        last = adv;
    }
}

__global__ void ev2g_gae_kernel(const double *reward, const float *values, const uint8_t *episode_starts, const float *last_values,
                                const uint8_t *last_dones, int k, int E, float g, float c, float *advantages, float *returns) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) ev2g_gae_env(reward, values, episode_starts, last_values, last_dones, k, E, e, g, c, advantages, returns);
}
