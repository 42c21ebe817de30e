// ev2g_ppo.h -- the learner of the Gaussian actor-critic (ev2g_ac.h): SB3's PPO.train() with default settings, one minibatch per call, and SB3's
// A2C.train(), one update over the rows it is given.  The two differ in the head of the gradient kernel (a compile-time choice) and the optimiser.
//
//   ev2g_ppo_advstat_kernel   mean and unbiased std of the minibatch's gathered advantages (one workgroup, float64, fixed order)
//   ev2g_ppo_grad_kernel      per 32 gathered rows: forward with every activation kept, the head gradients, backprop, weight gradients; a
//                             workgroup loops over its chunks and keeps its partial sums in a slab of its own in the workspace
//   ev2g_ppo_reduce_kernel    sums the slabs in workgroup order (float64, rounded once) into the flat gradient, the statistics likewise, and
//                             writes one partial of the squared norm per block
//   ev2g_ppo_apply_kernel     sums those partials in block order, clips, Adam on the float32 masters ([out, in] row-major, SB3's layout), and
//                             rewrites the element's places in the packed images AcDev points at (pack_linear_f32's order; padding is never written)
//   ev2g_a2c_apply_kernel     the same with torch.optim.RMSprop in Adam's place (its square average lives in the learner's v buffer)
//
// No float atomics anywhere and every sum has one fixed order: the same call on the same state gives the same bits.  No kernel waits on another
// workgroup: the stages are separate launches on the handle's stream.
//
// Backprop needs delta_prev = (delta W) . act'(h): a product over a layer's OUTPUTS, so W2, W3 and the value trunk's second layer have a second
// image, pack_linear_f32 of the transpose.  The weight gradient dW = delta^T H is a 32 x 32 tile with K = the chunk's 32 rows, both operands
// read from LDS.  Rows past the end of a chunk have zero head gradients, hence zero deltas, hence add exact zeros.
#pragma once

struct PpoHyper { float clip, vf_coef, ent_coef; int normalize; };

// ---- element functions: host (ev2g_host_ppo_head, ev2g_host_adam) and device from this source ----
#define EV2G_HALF_LOG_2PI 0.9189385332046727

// ports j, j + step, ... of one row's log-probability terms; iv[p] = exp(-2 log_std[p])
__host__ __device__ inline double ev2g_ppo_lp_part(const float *mu, const float *a, const float *log_std, const double *iv, int P, int j, int step) {
    double lp = 0.0;
    for (int p = j; p < P; p += step) {
        const double d = (double)a[p] - (double)mu[p];
        lp += -(d * d) * (0.5 * iv[p]) - (double)log_std[p] - EV2G_HALF_LOG_2PI;
    }
    return lp;
}

// the eight partial sums of a row meet as the device's butterfly joins them (xor 4, 2, 1)
__host__ __device__ inline double ev2g_ppo_join8(const double *q) { return ((q[0] + q[4]) + (q[2] + q[6])) + ((q[1] + q[5]) + (q[3] + q[7])); }

struct PpoRow {
    float g_lp, g_v;               // d loss / d lp_i, d loss / d v_i
    double pol, vsq, kl, clipped;  // this row's terms of policy_loss (before the minus), value_loss, approx_kl, clip_fraction
};
// one row's head: lp its log-probability, adv the (normalised) advantage
__host__ __device__ inline PpoRow ev2g_ppo_head_row(double lp, float old_lp, float adv, float ret, float v, float clip, float vf_coef, double inv_b) {
    PpoRow o;
    const double lr = lp - (double)old_lp, r = exp(lr), A = (double)adv, c = (double)clip;
    const double rc = r < 1.0 - c ? 1.0 - c : (r > 1.0 + c ? 1.0 + c : r);
    const double s1 = A * r, s2 = A * rc;
    o.pol = s1 < s2 ? s1 : s2;
    // what torch.min / torch.clamp backpropagate, ties included: the unclipped branch unless the clipped one is strictly smaller
    const bool open = (A >= 0.0 && r <= 1.0 + c) || (A < 0.0 && r >= 1.0 - c);
    o.g_lp = open ? (float)(-A * r * inv_b) : 0.0f;
    const double dv = (double)v - (double)ret;
    o.vsq = dv * dv;
    o.g_v = (float)(2.0 * (double)vf_coef * dv * inv_b);
    o.kl = (r - 1.0) - lr;
    o.clipped = fabs(r - 1.0) > c ? 1.0 : 0.0;
    return o;
}

// A2C's head of one row: no ratio and no clip, policy_loss = -mean(A lp); the two ratio statistics are exact zeros
__host__ __device__ inline PpoRow ev2g_a2c_head_row(double lp, float adv, float ret, float v, float vf_coef, double inv_b) {
    PpoRow o;
    const double A = (double)adv;
    o.pol = A * lp;
    o.g_lp = (float)(-A * inv_b);
    const double dv = (double)v - (double)ret;
    o.vsq = dv * dv;
    o.g_v = (float)(2.0 * (double)vf_coef * dv * inv_b);
    o.kl = 0.0;
    o.clipped = 0.0;
    return o;
}

// one (row, port): d loss / d mean and the row's term of d loss / d log_std
__host__ __device__ inline void ev2g_ppo_head_port(float a, float mu, double iv, float g_lp, float *d_mu, float *d_ls) {
    const double d = (double)a - (double)mu;
    *d_mu = (float)((double)g_lp * (d * iv));
    *d_ls = (float)((double)g_lp * (d * d * iv - 1.0));
}

// the six statistics from the minibatch's sums (pol, vsq, kl, clipped) and the master log_std
__host__ __device__ inline void ev2g_ppo_stats(const double *sum, const float *log_std, int P, double inv_b, float vf_coef, float ent_coef, float *stats) {
    double ent = 0.0;
    for (int p = 0; p < P; p++) ent += 0.5 + EV2G_HALF_LOG_2PI + (double)log_std[p];
    const double pl = -sum[0] * inv_b, vl = sum[1] * inv_b, el = -ent;
    stats[0] = (float)pl; stats[1] = (float)vl; stats[2] = (float)el;
    stats[3] = (float)(pl + (double)ent_coef * el + (double)vf_coef * vl);
    stats[4] = (float)(sum[2] * inv_b); stats[5] = (float)(sum[3] * inv_b);
}

// torch.optim.Adam's step of one element (no amsgrad, no weight decay): step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t); omb1 / omb2
// are 1 - beta1 / 1 - beta2 rounded from float64 (1.0f - beta2 would carry beta2's rounding error at a relative 5e-5).  m moves as torch's
// lerp_ moves it, v as mul_ then addcmul_.
struct AdamStep { float omb1, beta2, omb2, step_size, bc2_sqrt, eps; };
__host__ __device__ inline void ev2g_adam_elem(float *theta, float *m, float *v, float g, const AdamStep &a) {
    const float omb1 = a.omb1, beta2 = a.beta2, omb2 = a.omb2, step_size = a.step_size, bc2_sqrt = a.bc2_sqrt, eps = a.eps;
    const float mn = *m + omb1 * (g - *m);
    const float vn = beta2 * *v + (omb2 * g) * g;
    *m = mn; *v = vn;
    const float denom = sqrtf(vn) / bc2_sqrt + eps;
    *theta = *theta - step_size * (mn / denom);
}

// torch.optim.RMSprop's step of one element (no weight decay, no momentum, not centered): sq moves as mul_ then addcmul_ (oma is 1 - alpha
// rounded from float64, as for Adam), the denominator is sqrt().add_(eps), theta moves as addcdiv_ with value -lr: (lr g) / avg.
struct RmsStep { float alpha, oma, lr, eps; };
__host__ __device__ inline void ev2g_rmsprop_elem(float *theta, float *sq, float g, const RmsStep &s) {
    const float alpha = s.alpha, oma = s.oma, lr = s.lr, eps = s.eps;
    const float sn = alpha * *sq + (oma * g) * g;
    *sq = sn;
    const float avg = sqrtf(sn) + eps;
    *theta = *theta - (lr * g) / avg;
}

#ifdef __HIPCC__
// ---- the advantage statistics of a minibatch: out[0] = mean, out[1] = 1 / (unbiased std + 1e-8) ----
__global__ void __launch_bounds__(1024) ev2g_ppo_advstat_kernel(const float *__restrict__ adv, const int *__restrict__ idx, int B, double *__restrict__ out) {
    __shared__ double red[1024];
    __shared__ double mean_s;
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < B; i += 1024) s += (double)adv[idx[i]];
    red[t] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) mean_s = red[0] / (double)B;
    __syncthreads();
    const double mean = mean_s;
    s = 0.0;
    for (int i = t; i < B; i += 1024) { const double d = (double)adv[idx[i]] - mean; s += d * d; }
    __syncthreads();
    red[t] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) { out[0] = mean; out[1] = 1.0 / (sqrt(red[0] / (double)(B - 1)) + 1e-8); }
}

// what the gradient kernel reads besides the network: the transposed images and the master log_std
struct PpoDev {
    int k1r;                            // the first layers' inputs padded to 32 (the x block's zero-filled width)
    const float *w2t, *w3t, *u2t;       // pack_linear_f32 of W2^T [n1 <- n2], W3^T [n2 <- n3], U2^T [m1 <- m2]
    const float *log_std;               // [P], the master
    int slab_off[EV2G_PPO_ARRAYS], slab_floats;
};

// one 32-column tile of delta_prev = (delta Wt^T) . act'(h) for the workgroup's 32 rows: ev2g_ac_tile's k-ordered chain with another epilogue
template <int ACT>
__device__ __forceinline__ void ev2g_ppo_back_tile(const float *__restrict__ A, int sa, int KG, const float *__restrict__ Wt, int col0,
                                                   const float *__restrict__ H, int sh, float *__restrict__ out, int so) {
    const int lane = threadIdx.x & 63;
    const float *arow = A + (lane & 31) * sa + 4 * (lane >> 5);
    const f32x4 *w = (const f32x4 *)Wt + lane;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int g = 0; g < KG; g++) {
        const f32x4 a = *(const f32x4 *)(arow + g * 8), b = w[(size_t)g * 64];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
    const int col = col0 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const float h = H[row * sh + col];
        const float d = ACT == EV2G_AC_TANH ? 1.0f - h * h : (h > 0.0f ? 1.0f : 0.0f);
        out[row * so + col] = acc[r] * d;
    }
}

// one 32 x 32 tile of dW += delta^T H over the chunk's 32 rows: element (n0 + i, k0 + j) = sum_row D[row][n0 + i] Hb[row][k0 + j], rows
// ascending in pairs (MFMA q takes rows 2 q and 2 q + 1); the running sum lives in the workgroup's slab [.][ld]
__device__ __forceinline__ void ev2g_ppo_dw_tile(const float *__restrict__ D, int sd, int n0, const float *__restrict__ Hb, int sh, int k0,
                                                 float *__restrict__ slab, int ld, bool first) {
    const int lane = threadIdx.x & 63;
    const float *dp = D + (lane >> 5) * sd + n0 + (lane & 31), *hp = Hb + (lane >> 5) * sh + k0 + (lane & 31);
    float *dst = slab + (size_t)(n0 + 4 * (lane >> 5)) * ld + k0 + (lane & 31);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = first ? 0.0f : dst[(size_t)((r & 3) + 8 * (r >> 2)) * ld];
#pragma unroll
    for (int q = 0; q < EV2G_PPO_ROWS / 2; q++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dp[2 * q * sd], hp[2 * q * sh], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; r++) dst[(size_t)((r & 3) + 8 * (r >> 2)) * ld] = acc[r];
}

// column sums of a delta block over the 32 rows (rows ascending), added to the slab's bias gradient
__device__ __forceinline__ void ev2g_ppo_colsum(const float *__restrict__ D, int sd, int n, float *__restrict__ slab, bool first) {
    for (int c = threadIdx.x; c < n; c += EV2G_PPO_BLOCK) {
        float s = first ? 0.0f : slab[c];
        for (int r = 0; r < EV2G_PPO_ROWS; r++) s += D[r * sd + c];
        slab[c] = s;
    }
}

// HEAD: the loss of a row, a compile-time choice.  EV2G_HEAD_A2C reads no old_lp (the host passes null).
#define EV2G_HEAD_PPO 0
#define EV2G_HEAD_A2C 1
template <int ACT, int HEAD>
__global__ void __launch_bounds__(EV2G_PPO_BLOCK) ev2g_ppo_grad_kernel(AcDev m, PpoDev q, PpoLds L, PpoHyper hp, const float *__restrict__ obs,
                                                                     const float *__restrict__ actions, const float *__restrict__ old_lp,
                                                                     const float *__restrict__ adv, const float *__restrict__ ret,
                                                                     const int *__restrict__ idx, int B, const double *__restrict__ advstat,
                                                                     float *__restrict__ work, double *__restrict__ stat_part) {
    extern __shared__ __attribute__((aligned(16))) float ppo_lds_mem[];
    float *base = ppo_lds_mem;
    double *iv = (double *)(base + L.oIV);
    float *X = base + L.oX, *H1 = base + L.oH1, *H2 = base + L.oH2, *V1 = base + L.oV1, *V2 = base + L.oV2, *MU = base + L.oMU, *ACTN = base + L.oACT;
    float *D1 = base + L.oD1, *D2 = base + L.oD2, *E1 = base + L.oE1, *E2 = base + L.oE2;
    float *g_lp = base + L.oROW, *g_v = g_lp + EV2G_PPO_ROWS;
    const int wave = threadIdx.x >> 6, NW = EV2G_PPO_BLOCK / 64;
    const int P = m.d_out;
    float *slab = work + (size_t)blockIdx.x * q.slab_floats;
    const int n_chunks = (B + EV2G_PPO_ROWS - 1) / EV2G_PPO_ROWS;
    const double inv_b = 1.0 / (double)B;
    const bool norm = hp.normalize && B > 1;
    const double a_mean = norm ? advstat[0] : 0.0, a_scale = norm ? advstat[1] : 1.0;
    for (int p = threadIdx.x; p < m.n3; p += EV2G_PPO_BLOCK) iv[p] = p < P ? exp(-2.0 * (double)q.log_std[p]) : 0.0;
    double st0 = 0.0, st1 = 0.0, st2 = 0.0, st3 = 0.0;   // this lane's rows' statistics terms (lanes with j == 0)
    bool first = true;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x, first = false) {
        const int row0 = chunk * EV2G_PPO_ROWS;
        const int nr = B - row0 < EV2G_PPO_ROWS ? B - row0 : EV2G_PPO_ROWS;
        __syncthreads();   // the previous chunk's readers are done with every block
        // gathered rows -> LDS, zeros past the last row and past D (up to the 32-padded width) / P
        for (int i = threadIdx.x; i < EV2G_PPO_ROWS * q.k1r; i += EV2G_PPO_BLOCK) {
            const int r = i / q.k1r, c = i - r * q.k1r;
            X[r * L.sX + c] = (r < nr && c < m.d_in) ? obs[(size_t)idx[row0 + r] * m.d_in + c] : 0.0f;
        }
        for (int i = threadIdx.x; i < EV2G_PPO_ROWS * m.n3; i += EV2G_PPO_BLOCK) {
            const int r = i / m.n3, c = i - r * m.n3;
            ACTN[r * L.sMU + c] = (r < nr && c < P) ? actions[(size_t)idx[row0 + r] * P + c] : 0.0f;
        }
        __syncthreads();
        {   // forward, as ev2g_ac_act_kernel, every activation kept: X -> H1 -> H2 -> MU, X -> V1 -> V2
            const int KG = m.k1 >> 3, tp = m.n1 >> 5, tv = m.m1 >> 5;
            for (int t = wave; t < tp + tv; t += NW) {
                if (t < tp) ev2g_ac_tile<ACT>(X, L.sX, KG, m.w1 + (size_t)t * KG * 256, m.b1, t * 32, H1, L.sH1);
                else ev2g_ac_tile<ACT>(X, L.sX, KG, m.u1 + (size_t)(t - tp) * KG * 256, m.c1, (t - tp) * 32, V1, L.sV1);
            }
        }
        __syncthreads();
        {
            const int KGp = m.n1 >> 3, KGv = m.m1 >> 3, tp = m.n2 >> 5, tv = m.m2 >> 5;
            for (int t = wave; t < tp + tv; t += NW) {
                if (t < tp) ev2g_ac_tile<ACT>(H1, L.sH1, KGp, m.w2 + (size_t)t * KGp * 256, m.b2, t * 32, H2, L.sH2);
                else ev2g_ac_tile<ACT>(V1, L.sV1, KGv, m.u2 + (size_t)(t - tp) * KGv * 256, m.c2, (t - tp) * 32, V2, L.sV2);
            }
        }
        __syncthreads();
        {
            const int KG = m.n2 >> 3, tp = m.n3 >> 5;
            for (int t = wave; t < tp; t += NW) ev2g_ac_tile<EV2G_AC_LINEAR>(H2, L.sH2, KG, m.w3 + (size_t)t * KG * 256, m.b3, t * 32, MU, L.sMU);
        }
        __syncthreads();
        {   // heads: eight lanes per row (lane j takes k / p = j, j + 8, ...), a fixed butterfly
            const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
            float pv = 0.0f;
            for (int k = j; k < m.m2; k += 8) pv = fmaf(V2[row * L.sV2 + k], m.u3[k], pv);
            pv += __shfl_xor(pv, 4); pv += __shfl_xor(pv, 2); pv += __shfl_xor(pv, 1);
            pv += m.c3[0];
            double lp = ev2g_ppo_lp_part(MU + row * L.sMU, ACTN + row * L.sMU, q.log_std, iv, P, j, 8);
            lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 1);
            if (j == 0) {
                float gl = 0.0f, gv = 0.0f;
                if (row < nr) {
                    const int i = idx[row0 + row];
                    const float A = norm ? (float)(((double)adv[i] - a_mean) * a_scale) : adv[i];
                    const PpoRow o = HEAD == EV2G_HEAD_PPO ? ev2g_ppo_head_row(lp, old_lp[i], A, ret[i], pv, hp.clip, hp.vf_coef, inv_b)
                                                           : ev2g_a2c_head_row(lp, A, ret[i], pv, hp.vf_coef, inv_b);
                    gl = o.g_lp; gv = o.g_v;
                    st0 += o.pol; st1 += o.vsq; st2 += o.kl; st3 += o.clipped;
                }
                g_lp[row] = gl; g_v[row] = gv;
            }
        }
        __syncthreads();
        // d loss / d log_std: each port's 32 row terms summed rows ascending (read before MU becomes d loss / d mean)
        for (int p = threadIdx.x; p < P; p += EV2G_PPO_BLOCK) {
            float *dst = slab + q.slab_off[12] + p;
            float s = first ? 0.0f : *dst, dm, dl;
            for (int r = 0; r < EV2G_PPO_ROWS; r++) {
                ev2g_ppo_head_port(ACTN[r * L.sMU + p], MU[r * L.sMU + p], iv[p], g_lp[r], &dm, &dl);
                s += dl;
            }
            *dst = s;
        }
        __syncthreads();
        // MU <- d loss / d mean (zeros past P); E2 <- delta of the value trunk's second layer (elementwise: the head is one row)
        for (int i = threadIdx.x; i < EV2G_PPO_ROWS * m.n3; i += EV2G_PPO_BLOCK) {
            const int r = i / m.n3, c = i - r * m.n3;
            float dm = 0.0f, dl;
            if (c < P) ev2g_ppo_head_port(ACTN[r * L.sMU + c], MU[r * L.sMU + c], iv[c], g_lp[r], &dm, &dl);
            MU[r * L.sMU + c] = dm;
        }
        for (int i = threadIdx.x; i < EV2G_PPO_ROWS * m.m2; i += EV2G_PPO_BLOCK) {
            const int r = i / m.m2, c = i - r * m.m2;
            const float h = V2[r * L.sV2 + c];
            const float d = ACT == EV2G_AC_TANH ? 1.0f - h * h : (h > 0.0f ? 1.0f : 0.0f);
            E2[r * L.sV2 + c] = (g_v[r] * m.u3[c]) * d;
        }
        __syncthreads();
        {   // D2 = (dMU W3) . act'(H2)
            const int KG = m.n3 >> 3, tp = m.n2 >> 5;
            for (int t = wave; t < tp; t += NW) ev2g_ppo_back_tile<ACT>(MU, L.sMU, KG, q.w3t + (size_t)t * KG * 256, t * 32, H2, L.sH2, D2, L.sH2);
        }
        __syncthreads();
        {   // D1 = (D2 W2) . act'(H1), E1 = (E2 U2) . act'(V1)
            const int KGp = m.n2 >> 3, KGv = m.m2 >> 3, tp = m.n1 >> 5, tv = m.m1 >> 5;
            for (int t = wave; t < tp + tv; t += NW) {
                if (t < tp) ev2g_ppo_back_tile<ACT>(D2, L.sH2, KGp, q.w2t + (size_t)t * KGp * 256, t * 32, H1, L.sH1, D1, L.sH1);
                else ev2g_ppo_back_tile<ACT>(E2, L.sV2, KGv, q.u2t + (size_t)(t - tp) * KGv * 256, (t - tp) * 32, V1, L.sV1, E1, L.sV1);
            }
        }
        __syncthreads();
        {   // the weight gradients: every 32 x 32 tile of the five matrices, shared out over the wavefronts
            const int kx = q.k1r >> 5, t1 = (m.n1 >> 5) * kx, t2 = (m.n2 >> 5) * (m.n1 >> 5), t3 = (m.n3 >> 5) * (m.n2 >> 5), t4 = (m.m1 >> 5) * kx,
                      t5 = (m.m2 >> 5) * (m.m1 >> 5);
            for (int t = wave; t < t1 + t2 + t3 + t4 + t5; t += NW) {
                int u = t;
                if (u < t1) { ev2g_ppo_dw_tile(D1, L.sH1, (u / kx) * 32, X, L.sX, (u % kx) * 32, slab + q.slab_off[0], q.k1r, first); continue; }
                u -= t1;
                if (u < t2) { const int kn = m.n1 >> 5; ev2g_ppo_dw_tile(D2, L.sH2, (u / kn) * 32, H1, L.sH1, (u % kn) * 32, slab + q.slab_off[2], m.n1, first); continue; }
                u -= t2;
                if (u < t3) { const int kn = m.n2 >> 5; ev2g_ppo_dw_tile(MU, L.sMU, (u / kn) * 32, H2, L.sH2, (u % kn) * 32, slab + q.slab_off[8], m.n2, first); continue; }
                u -= t3;
                if (u < t4) { ev2g_ppo_dw_tile(E1, L.sV1, (u / kx) * 32, X, L.sX, (u % kx) * 32, slab + q.slab_off[4], q.k1r, first); continue; }
                u -= t4;
                { const int kn = m.m1 >> 5; ev2g_ppo_dw_tile(E2, L.sV2, (u / kn) * 32, V1, L.sV1, (u % kn) * 32, slab + q.slab_off[6], m.m1, first); }
            }
            // the bias gradients and the value head's: column sums of the deltas, g_v^T V2, sum g_v
            ev2g_ppo_colsum(D1, L.sH1, m.n1, slab + q.slab_off[1], first);
            ev2g_ppo_colsum(D2, L.sH2, m.n2, slab + q.slab_off[3], first);
            ev2g_ppo_colsum(E1, L.sV1, m.m1, slab + q.slab_off[5], first);
            ev2g_ppo_colsum(E2, L.sV2, m.m2, slab + q.slab_off[7], first);
            ev2g_ppo_colsum(MU, L.sMU, m.n3, slab + q.slab_off[9], first);
            for (int c = threadIdx.x; c < m.m2; c += EV2G_PPO_BLOCK) {
                float *dst = slab + q.slab_off[10] + c;
                float s = first ? 0.0f : *dst;
                for (int r = 0; r < EV2G_PPO_ROWS; r++) s += g_v[r] * V2[r * L.sV2 + c];
                *dst = s;
            }
            if (threadIdx.x == EV2G_PPO_BLOCK - 1) {
                float *dst = slab + q.slab_off[11];
                float s = first ? 0.0f : *dst;
                for (int r = 0; r < EV2G_PPO_ROWS; r++) s += g_v[r];
                *dst = s;
            }
        }
    }
    // the workgroup's statistics: row r's lane (thread 8 r) holds its rows' terms; summed rows ascending by one thread
    __syncthreads();
    double *sred = (double *)(base + L.oX);   // (X is free now; its offset is a multiple of two floats past a 16-byte aligned base)
    if ((threadIdx.x & 7) == 0) {
        const int r = threadIdx.x >> 3;
        sred[r * 4 + 0] = st0; sred[r * 4 + 1] = st1; sred[r * 4 + 2] = st2; sred[r * 4 + 3] = st3;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = 0.0;
        for (int r = 0; r < EV2G_PPO_ROWS; r++) s += sred[r * 4 + threadIdx.x];
        stat_part[(size_t)blockIdx.x * 8 + threadIdx.x] = s;
    }
}

// PpoMap (ev2g_policy_host.h: ppo_map builds it on the host) says where the thirteen arrays sit: the flat buffers, the slabs, the packed images
__device__ __forceinline__ int ev2g_ppo_which(const PpoMap &mp, int i) {
    int a = 0;
#pragma unroll
    for (int k = 1; k < EV2G_PPO_ARRAYS; k++) a += i >= mp.off[k] ? 1 : 0;
    return a;
}

// flat gradient element i = the sum over the n_wg slabs, workgroups ascending, in float64, rounded once; block b's sum of squares -> norm_part[b];
// block 0 also sums the statistics partials and writes the six statistics (stats may be null)
__global__ void __launch_bounds__(256) ev2g_ppo_reduce_kernel(PpoMap mp, const float *__restrict__ work, const double *__restrict__ stat_part, int n_wg,
                                                            int B, PpoHyper hp, const float *__restrict__ log_std, float *__restrict__ grad,
                                                            double *__restrict__ norm_part, float *__restrict__ stats) {
    __shared__ double red[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double sq = 0.0;
    if (i < mp.n_params) {
        const int a = ev2g_ppo_which(mp, i), e = i - mp.off[a];
        const int r = e / mp.cols[a], c = e - r * mp.cols[a];
        const float *src = work + mp.slab_off[a] + (size_t)r * mp.slab_ld[a] + c;
        double s = 0.0;
        for (int w = 0; w < n_wg; w++) s += (double)src[(size_t)w * mp.slab_floats];
        if (a == 12) s -= (double)hp.ent_coef;   // the entropy term's share of d loss / d log_std
        const float g = (float)s;
        grad[i] = g;
        sq = (double)g * (double)g;
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) norm_part[blockIdx.x] = red[0];
    if (blockIdx.x == 0 && threadIdx.x == 0 && stats) {
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < n_wg; w++)
            for (int k = 0; k < 4; k++) sum[k] += stat_part[(size_t)w * 8 + k];
        ev2g_ppo_stats(sum, log_std, mp.P, 1.0 / (double)B, hp.vf_coef, hp.ent_coef, stats);
    }
}

// clip_grad_norm_'s coefficient from the reduce kernel's partials, summed in block order (thread 0 of every block; the others read coef_s after the barrier)
__device__ __forceinline__ void ev2g_ppo_clip_coef(const double *__restrict__ norm_part, int n_blocks, float max_grad_norm, float *coef_s) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < n_blocks; b++) s += norm_part[b];
        const float norm = (float)sqrt(s);
        const float coef = max_grad_norm / (norm + 1e-6f);
        *coef_s = coef < 1.0f ? coef : 1.0f;
    }
    __syncthreads();
}

// the new value t of master element i into its places in the packed image and the transposed image
__device__ __forceinline__ void ev2g_ppo_place(const PpoMap &mp, int i, float t) {
    const int a = ev2g_ppo_which(mp, i), e = i - mp.off[a];
    if (!mp.img[a]) return;
    if (mp.img_k[a] == 0) { mp.img[a][e] = t; return; }
    const int r = e / mp.cols[a], c = e - r * mp.cols[a];
    mp.img[a][packed_f32_index(r, c, mp.img_k[a])] = t;
    if (mp.imgT[a]) mp.imgT[a][packed_f32_index(c, r, mp.imgT_k[a])] = t;
}

// clip_grad_norm_ and Adam on element i of the masters, and the element's places in the packed images
__global__ void __launch_bounds__(256) ev2g_ppo_apply_kernel(PpoMap mp, const float *__restrict__ grad, const double *__restrict__ norm_part, int n_blocks,
                                                           float max_grad_norm, AdamStep adam, float *__restrict__ theta, float *__restrict__ am, float *__restrict__ av) {
    __shared__ float coef_s;
    ev2g_ppo_clip_coef(norm_part, n_blocks, max_grad_norm, &coef_s);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= mp.n_params) return;
    float t = theta[i], mm = am[i], vv = av[i];
    ev2g_adam_elem(&t, &mm, &vv, grad[i] * coef_s, adam);
    theta[i] = t; am[i] = mm; av[i] = vv;
    ev2g_ppo_place(mp, i, t);
}

// clip_grad_norm_ and RMSprop on element i of the masters (sq: the learner's v buffer), and the element's places in the packed images
__global__ void __launch_bounds__(256) ev2g_a2c_apply_kernel(PpoMap mp, const float *__restrict__ grad, const double *__restrict__ norm_part, int n_blocks,
                                                           float max_grad_norm, RmsStep rms, float *__restrict__ theta, float *__restrict__ sq) {
    __shared__ float coef_s;
    ev2g_ppo_clip_coef(norm_part, n_blocks, max_grad_norm, &coef_s);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= mp.n_params) return;
    float t = theta[i], s = sq[i];
    ev2g_rmsprop_elem(&t, &s, grad[i] * coef_s, rms);
    theta[i] = t; sq[i] = s;
    ev2g_ppo_place(mp, i, t);
}

// masters -> images for every element (ev2g_ppo_create, and ev2g_ac_set_weights on a bound policy, refresh the transposed images by it)
__global__ void __launch_bounds__(256) ev2g_ppo_repack_kernel(PpoMap mp, const float *__restrict__ theta, int transposed_only) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= mp.n_params) return;
    const int a = ev2g_ppo_which(mp, i), e = i - mp.off[a];
    if (!mp.img[a]) return;
    const float t = theta[i];
    if (mp.img_k[a] == 0) { if (!transposed_only) mp.img[a][e] = t; return; }
    const int r = e / mp.cols[a], c = e - r * mp.cols[a];
    if (!transposed_only) mp.img[a][packed_f32_index(r, c, mp.img_k[a])] = t;
    if (mp.imgT[a]) mp.imgT[a][packed_f32_index(c, r, mp.imgT_k[a])] = t;
}
#endif
