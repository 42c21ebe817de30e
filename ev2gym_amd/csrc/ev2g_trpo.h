// ev2g_trpo.h -- the third learner of the Gaussian actor-critic (ev2g_ac.h): sb3_contrib's TRPO.train() with default settings.  A natural-gradient
// policy step over the rows it is given (objective gradient, conjugate gradient on Fisher-vector products, backtracking line search), queued
// on the handle's stream without one host round trip, and Adam minibatches on the value trunk alone.
//
//   ev2g_trpo_policy_kernel<ACT, MODE>   per 32 gathered rows, the policy trunk only.  GRAD: forward, the head d J / d lp = A^ r / B, backprop, weight
//                             gradients into the workgroup's slab; stores mu0 [B, P] and the workgroup's partial of J.  FVP: forward keeping H1 and
//                             H2, the tangent pass along a direction (T1, T2, Tmu), Tmu scaled by exp(-2 log_std) / B, then the same backprop and
//                             weight-gradient tiles (ev2g_ppo_back_tile / _dw_tile / _colsum).  EVAL: forward, lp, r, and the workgroup's partials of
//                             J and KL against the stored mu0 / log_std0.
//   ev2g_trpo_value_kernel<ACT>   the value trunk only: forward, the head d/dv = 2 (v - R) / B, backprop, weight gradients, the partial of value_loss
//   ev2g_trpo_reduce_kernel   slabs -> a flat actor vector (float64 sums, workgroups ascending); a Fisher product gets 2 v on the log_std block and
//                             damping v everywhere (the log_std block of the Fisher matrix is exactly 2 I: no slab is read for it)
//   ev2g_trpo_dir_kernel      a flat actor vector -> the direction images
//   ev2g_trpo_cg_init / _cg_step / _stepsize / _decide   one workgroup each: the dots in float64 (a thread's strided partial, then a fixed tree),
//                             alpha, x, r, rho, p, the 1e-10 exits, beta, and the line search's accept / shrink / restore
//   ev2g_trpo_candidate_kernel   theta0 + c beta x into the float32 masters and their places in the packed and transposed images
//   ev2g_trpo_vreduce / _vapply   the six value arrays' gradient and their Adam step (no clip); nothing else is touched
//
// The rules are ev2g_ppo.h's: float32 operands on the exact-f32 MFMA, float64 in heads and sums, no float atomics, every sum in one fixed order,
// no kernel waits on another workgroup.  The conjugate-gradient vectors (g, x, r, p, Hv) are kept in float64: they ARE sums, 15 iterations deep
// (p holds float32 values: see ev2g_trpo_cg_init_kernel).
//
// The direction's three matrices are read as the MFMA's B operand from DIRECTION IMAGES in pack_linear_f32 order, written by ev2g_trpo_dir_kernel
// before each product: the tangent tiles then run ev2g_ac_tile's k-ordered chain on 16-byte lane loads, as the forward does on the weights.
// Reading the flat [out, in] rows directly would make every lane's load a strided gather of single floats per MFMA; the repack is one pass over
// the vector per product.
//
// The state of a step (TrpoState) lives on the device.  Once the solve has ended, the remaining queued iterations' launches read it and return at
// once; after an accepted try, the remaining tries likewise.  After the last failed try theta0 and its images are written back bit for bit.
// DEVIATION from sb3_contrib: a non-finite or non-positive x . Hx (a zero gradient's x = 0 included: the rho < 1e-10 exit before the first
// iteration) marks the step failed and leaves theta0 in place; sb3_contrib would write NaN parameters.
#pragma once

#define EV2G_TRPO_RHO_MIN 1e-10

// ---- element functions: host (ev2g_host_trpo_rows) and device from this source ----
// KL(N(mu, e^ls) || N(mu0, e^ls0)) of one port = kc + kq (mu - mu0)^2 with kc = ls0 - ls + e^{2 ls} / (2 e^{2 ls0}) - 1/2, kq = 1 / (2 e^{2 ls0})
__host__ __device__ inline void ev2g_trpo_kl_consts(float ls, float ls0, double *kc, double *kq) {
    const double q = 0.5 * exp(-2.0 * (double)ls0);
    *kq = q;
    *kc = (double)ls0 - (double)ls + exp(2.0 * (double)ls) * q - 0.5;
}
// ports j, j + step, ... of one row's KL
__host__ __device__ inline double ev2g_trpo_kl_part(const float *mu, const float *mu0, const double *kc, const double *kq, int P, int j, int step) {
    double s = 0.0;
    for (int p = j; p < P; p += step) {
        const double d = (double)mu[p] - (double)mu0[p];
        s += kc[p] + kq[p] * (d * d);
    }
    return s;
}

#ifdef __HIPCC__
#define EV2G_TRPO_GRAD 0
#define EV2G_TRPO_FVP 1
#define EV2G_TRPO_EVAL 2
#define EV2G_TRPO_GATE_NONE 0
#define EV2G_TRPO_GATE_CG 1   // return at once when the solve has ended
#define EV2G_TRPO_GATE_LS 2   // ... when the line search has

struct TrpoArgs {
    const float *obs, *actions, *old_lp, *adv, *ret;
    const int *idx;
    int B, normalize;
    const double *advstat;
    float *work;                // the slabs
    double *part;               // [grid][2]: the workgroup's partials (J, KL; the critic: the squared error)
    float *mu0;                 // [B, P]: GRAD writes it, EVAL reads it
    const float *ls0;           // [P]: log_std at theta0 (EVAL)
    const float *dw1, *db1, *dw2, *db2, *dw3, *db3;   // the direction images (FVP)
    const TrpoState *st;
    int gate;
};

__device__ __forceinline__ bool ev2g_trpo_gated(const TrpoState *st, int gate) {
    return (gate == EV2G_TRPO_GATE_CG && st->cg_done) || (gate == EV2G_TRPO_GATE_LS && st->ls_done);
}

// one 32-column tile of a tangent layer for the workgroup's 32 rows: acc = A1 . W1^T + A2 . W2^T (+ bias), both chains k ascending; hidden layers
// (ACT tanh / relu) multiply by act'(H); the linear head scales column c by scale[c] and zeroes rows >= nr and columns >= P
template <int ACT>
__device__ __forceinline__ void ev2g_trpo_tan_tile(const float *__restrict__ A1, int sa1, int KG1, const float *__restrict__ W1t, const float *__restrict__ A2,
                                                   int sa2, int KG2, const float *__restrict__ W2t, const float *__restrict__ bias, int col0,
                                                   const float *__restrict__ H, int sh, float *__restrict__ out, int so, const double *__restrict__ iv,
                                                   double inv_b, int nr, int P) {
    const int lane = threadIdx.x & 63;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    {
        const float *arow = A1 + (lane & 31) * sa1 + 4 * (lane >> 5);
        const f32x4 *w = (const f32x4 *)W1t + lane;
        for (int g = 0; g < KG1; g++) {
            const f32x4 a = *(const f32x4 *)(arow + g * 8), b = w[(size_t)g * 64];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    if (KG2 > 0) {   // (uniform)
        const float *arow = A2 + (lane & 31) * sa2 + 4 * (lane >> 5);
        const f32x4 *w = (const f32x4 *)W2t + lane;
        for (int g = 0; g < KG2; g++) {
            const f32x4 a = *(const f32x4 *)(arow + g * 8), b = w[(size_t)g * 64];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    const int col = col0 + (lane & 31);
    const float bv = bias[col];
    const float scale = ACT == EV2G_AC_LINEAR ? (col < P ? (float)(iv[col] * inv_b) : 0.0f) : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const float t = acc[r] + bv;
        if (ACT == EV2G_AC_LINEAR) out[row * so + col] = row < nr ? t * scale : 0.0f;
        else {
            const float h = H[row * sh + col];
            const float d = ACT == EV2G_AC_TANH ? 1.0f - h * h : (h > 0.0f ? 1.0f : 0.0f);
            out[row * so + col] = t * d;
        }
    }
}

template <int ACT, int MODE>
__global__ void __launch_bounds__(EV2G_PPO_BLOCK) ev2g_trpo_policy_kernel(AcDev m, PpoDev q, TrpoLds L, TrpoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float trpo_lds_mem[];
    if (ev2g_trpo_gated(a.st, a.gate)) return;   // (uniform over the launch: nothing in it writes the state)
    float *base = trpo_lds_mem;
    double *iv = (double *)(base + L.oIV), *kc = (double *)(base + L.oKC), *kq = (double *)(base + L.oKQ);
    float *X = base + L.oX, *H1 = base + L.oH1, *H2 = base + L.oH2, *T1 = base + L.oT1, *T2 = base + L.oT2, *MU = base + L.oMU, *ACTN = base + L.oACT;
    float *g_lp = base + L.oROW;
    const int wave = threadIdx.x >> 6, NW = EV2G_PPO_BLOCK / 64;
    const int P = m.d_out, B = a.B;
    float *slab = a.work + (size_t)blockIdx.x * q.slab_floats;
    const int n_chunks = (B + EV2G_PPO_ROWS - 1) / EV2G_PPO_ROWS;
    const double inv_b = 1.0 / (double)B;
    const bool norm = a.normalize && B > 1;
    const double a_mean = (MODE != EV2G_TRPO_FVP && norm) ? a.advstat[0] : 0.0, a_scale = (MODE != EV2G_TRPO_FVP && norm) ? a.advstat[1] : 1.0;
    for (int p = threadIdx.x; p < m.n3; p += EV2G_PPO_BLOCK) {
        iv[p] = p < P ? exp(-2.0 * (double)q.log_std[p]) : 0.0;
        if (MODE == EV2G_TRPO_EVAL) {
            double c = 0.0, s = 0.0;
            if (p < P) ev2g_trpo_kl_consts(q.log_std[p], a.ls0[p], &c, &s);
            kc[p] = c; kq[p] = s;
        }
    }
    double st0 = 0.0, st1 = 0.0;
    bool first = true;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x, first = false) {
        const int row0 = chunk * EV2G_PPO_ROWS;
        const int nr = B - row0 < EV2G_PPO_ROWS ? B - row0 : EV2G_PPO_ROWS;
        __syncthreads();
        for (int i = threadIdx.x; i < EV2G_PPO_ROWS * q.k1r; i += EV2G_PPO_BLOCK) {
            const int r = i / q.k1r, c = i - r * q.k1r;
            X[r * L.sX + c] = (r < nr && c < m.d_in) ? a.obs[(size_t)a.idx[row0 + r] * m.d_in + c] : 0.0f;
        }
        if (MODE != EV2G_TRPO_FVP)
            for (int i = threadIdx.x; i < EV2G_PPO_ROWS * m.n3; i += EV2G_PPO_BLOCK) {
                const int r = i / m.n3, c = i - r * m.n3;
                ACTN[r * L.sMU + c] = (r < nr && c < P) ? a.actions[(size_t)a.idx[row0 + r] * P + c] : 0.0f;
            }
        __syncthreads();
        {
            const int KG = m.k1 >> 3, tp = m.n1 >> 5;
            for (int t = wave; t < tp; t += NW) ev2g_ac_tile<ACT>(X, L.sX, KG, m.w1 + (size_t)t * KG * 256, m.b1, t * 32, H1, L.sA);
        }
        __syncthreads();
        {
            const int KG = m.n1 >> 3, tp = m.n2 >> 5;
            for (int t = wave; t < tp; t += NW) ev2g_ac_tile<ACT>(H1, L.sA, KG, m.w2 + (size_t)t * KG * 256, m.b2, t * 32, H2, L.sB);
        }
        __syncthreads();
        if (MODE != EV2G_TRPO_FVP) {
            {
                const int KG = m.n2 >> 3, tp = m.n3 >> 5;
                for (int t = wave; t < tp; t += NW) ev2g_ac_tile<EV2G_AC_LINEAR>(H2, L.sB, KG, m.w3 + (size_t)t * KG * 256, m.b3, t * 32, MU, L.sMU);
            }
            __syncthreads();
            {   // heads: eight lanes per row, a fixed butterfly (as ev2g_ppo_grad_kernel)
                const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
                double lp = ev2g_ppo_lp_part(MU + row * L.sMU, ACTN + row * L.sMU, q.log_std, iv, P, j, 8);
                lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 1);
                double kl = 0.0;
                if (MODE == EV2G_TRPO_EVAL) {
                    const int rr = row < nr ? row0 + row : row0;   // (rows past the end read a valid row; their terms are dropped)
                    kl = ev2g_trpo_kl_part(MU + row * L.sMU, a.mu0 + (size_t)rr * P, kc, kq, P, j, 8);
                    kl += __shfl_xor(kl, 4); kl += __shfl_xor(kl, 2); kl += __shfl_xor(kl, 1);
                }
                if (j == 0) {
                    float gl = 0.0f;
                    if (row < nr) {
                        const int i = a.idx[row0 + row];
                        const float A = norm ? (float)(((double)a.adv[i] - a_mean) * a_scale) : a.adv[i];
                        const double r = exp(lp - (double)a.old_lp[i]);
                        st0 += (double)A * r; st1 += kl;
                        gl = (float)((double)A * r * inv_b);
                    }
                    g_lp[row] = gl;
                }
            }
            __syncthreads();
        }
        if (MODE == EV2G_TRPO_EVAL) continue;
        if (MODE == EV2G_TRPO_GRAD) {
            for (int i = threadIdx.x; i < nr * P; i += EV2G_PPO_BLOCK) {
                const int r = i / P, c = i - r * P;
                a.mu0[(size_t)(row0 + r) * P + c] = MU[r * L.sMU + c];
            }
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
            for (int i = threadIdx.x; i < EV2G_PPO_ROWS * m.n3; i += EV2G_PPO_BLOCK) {
                const int r = i / m.n3, c = i - r * m.n3;
                float dm = 0.0f, dl;
                if (c < P) ev2g_ppo_head_port(ACTN[r * L.sMU + c], MU[r * L.sMU + c], iv[c], g_lp[r], &dm, &dl);
                MU[r * L.sMU + c] = dm;
            }
            __syncthreads();
        } else {   // the tangent pass: T1 = (X V1^T + v_b1) . act'(H1), T2 = (T1 W2^T + H1 V2^T + v_b2) . act'(H2), MU = (T2 W3^T + H2 V3^T + v_b3) e^{-2 ls} / B
            {
                const int KG = m.k1 >> 3, tp = m.n1 >> 5;
                for (int t = wave; t < tp; t += NW)
                    ev2g_trpo_tan_tile<ACT>(X, L.sX, KG, a.dw1 + (size_t)t * KG * 256, nullptr, 0, 0, nullptr, a.db1, t * 32, H1, L.sA, T1, L.sA, iv, inv_b, nr, P);
            }
            __syncthreads();
            {
                const int KG = m.n1 >> 3, tp = m.n2 >> 5;
                for (int t = wave; t < tp; t += NW)
                    ev2g_trpo_tan_tile<ACT>(T1, L.sA, KG, m.w2 + (size_t)t * KG * 256, H1, L.sA, KG, a.dw2 + (size_t)t * KG * 256, a.db2, t * 32, H2, L.sB, T2, L.sB,
                                            iv, inv_b, nr, P);
            }
            __syncthreads();
            {
                const int KG = m.n2 >> 3, tp = m.n3 >> 5;
                for (int t = wave; t < tp; t += NW)
                    ev2g_trpo_tan_tile<EV2G_AC_LINEAR>(T2, L.sB, KG, m.w3 + (size_t)t * KG * 256, H2, L.sB, KG, a.dw3 + (size_t)t * KG * 256, a.db3, t * 32, nullptr, 0,
                                                       MU, L.sMU, iv, inv_b, nr, P);
            }
            __syncthreads();
        }
        {   // T2 <- D2 = (dMU W3) . act'(H2)
            const int KG = m.n3 >> 3, tp = m.n2 >> 5;
            for (int t = wave; t < tp; t += NW) ev2g_ppo_back_tile<ACT>(MU, L.sMU, KG, q.w3t + (size_t)t * KG * 256, t * 32, H2, L.sB, T2, L.sB);
        }
        __syncthreads();
        {   // T1 <- D1 = (D2 W2) . act'(H1)
            const int KG = m.n2 >> 3, tp = m.n1 >> 5;
            for (int t = wave; t < tp; t += NW) ev2g_ppo_back_tile<ACT>(T2, L.sB, KG, q.w2t + (size_t)t * KG * 256, t * 32, H1, L.sA, T1, L.sA);
        }
        __syncthreads();
        {
            const int kx = q.k1r >> 5, t1 = (m.n1 >> 5) * kx, t2 = (m.n2 >> 5) * (m.n1 >> 5), t3 = (m.n3 >> 5) * (m.n2 >> 5);
            for (int t = wave; t < t1 + t2 + t3; t += NW) {
                int u = t;
                if (u < t1) { ev2g_ppo_dw_tile(T1, L.sA, (u / kx) * 32, X, L.sX, (u % kx) * 32, slab + q.slab_off[0], q.k1r, first); continue; }
                u -= t1;
                if (u < t2) { const int kn = m.n1 >> 5; ev2g_ppo_dw_tile(T2, L.sB, (u / kn) * 32, H1, L.sA, (u % kn) * 32, slab + q.slab_off[2], m.n1, first); continue; }
                u -= t2;
                { const int kn = m.n2 >> 5; ev2g_ppo_dw_tile(MU, L.sMU, (u / kn) * 32, H2, L.sB, (u % kn) * 32, slab + q.slab_off[8], m.n2, first); }
            }
            ev2g_ppo_colsum(T1, L.sA, m.n1, slab + q.slab_off[1], first);
            ev2g_ppo_colsum(T2, L.sB, m.n2, slab + q.slab_off[3], first);
            ev2g_ppo_colsum(MU, L.sMU, m.n3, slab + q.slab_off[9], first);
        }
    }
    if (MODE == EV2G_TRPO_FVP) return;
    // the workgroup's partials of J and KL: row r's lane (thread 8 r) holds its rows' terms; summed rows ascending by one thread
    __syncthreads();
    double *sred = (double *)(base + L.oX);
    if ((threadIdx.x & 7) == 0) {
        const int r = threadIdx.x >> 3;
        sred[r * 2 + 0] = st0; sred[r * 2 + 1] = st1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = 0.0;
        for (int r = 0; r < EV2G_PPO_ROWS; r++) s += sred[r * 2 + threadIdx.x];
        a.part[(size_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
}

// the critic: the value trunk alone, d value_loss / d v_i = 2 (v_i - R_i) / B; V1 / V2 live in the A / B blocks, their deltas in T1 / T2
template <int ACT>
__global__ void __launch_bounds__(EV2G_PPO_BLOCK) ev2g_trpo_value_kernel(AcDev m, PpoDev q, TrpoLds L, TrpoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float trpo_lds_mem[];
    float *base = trpo_lds_mem;
    float *X = base + L.oX, *V1 = base + L.oH1, *V2 = base + L.oH2, *E1 = base + L.oT1, *E2 = base + L.oT2;
    float *g_v = base + L.oROW;
    const int wave = threadIdx.x >> 6, NW = EV2G_PPO_BLOCK / 64;
    const int B = a.B;
    float *slab = a.work + (size_t)blockIdx.x * q.slab_floats;
    const int n_chunks = (B + EV2G_PPO_ROWS - 1) / EV2G_PPO_ROWS;
    const double inv_b = 1.0 / (double)B;
    double st0 = 0.0;
    bool first = true;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x, first = false) {
        const int row0 = chunk * EV2G_PPO_ROWS;
        const int nr = B - row0 < EV2G_PPO_ROWS ? B - row0 : EV2G_PPO_ROWS;
        __syncthreads();
        for (int i = threadIdx.x; i < EV2G_PPO_ROWS * q.k1r; i += EV2G_PPO_BLOCK) {
            const int r = i / q.k1r, c = i - r * q.k1r;
            X[r * L.sX + c] = (r < nr && c < m.d_in) ? a.obs[(size_t)a.idx[row0 + r] * m.d_in + c] : 0.0f;
        }
        __syncthreads();
        {
            const int KG = m.k1 >> 3, tv = m.m1 >> 5;
            for (int t = wave; t < tv; t += NW) ev2g_ac_tile<ACT>(X, L.sX, KG, m.u1 + (size_t)t * KG * 256, m.c1, t * 32, V1, L.sA);
        }
        __syncthreads();
        {
            const int KG = m.m1 >> 3, tv = m.m2 >> 5;
            for (int t = wave; t < tv; t += NW) ev2g_ac_tile<ACT>(V1, L.sA, KG, m.u2 + (size_t)t * KG * 256, m.c2, t * 32, V2, L.sB);
        }
        __syncthreads();
        {
            const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
            float pv = 0.0f;
            for (int k = j; k < m.m2; k += 8) pv = fmaf(V2[row * L.sB + k], m.u3[k], pv);
            pv += __shfl_xor(pv, 4); pv += __shfl_xor(pv, 2); pv += __shfl_xor(pv, 1);
            pv += m.c3[0];
            if (j == 0) {
                float gv = 0.0f;
                if (row < nr) {
                    const double dv = (double)pv - (double)a.ret[a.idx[row0 + row]];
                    st0 += dv * dv;
                    gv = (float)(2.0 * dv * inv_b);
                }
                g_v[row] = gv;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < EV2G_PPO_ROWS * m.m2; i += EV2G_PPO_BLOCK) {
            const int r = i / m.m2, c = i - r * m.m2;
            const float h = V2[r * L.sB + c];
            const float d = ACT == EV2G_AC_TANH ? 1.0f - h * h : (h > 0.0f ? 1.0f : 0.0f);
            E2[r * L.sB + c] = (g_v[r] * m.u3[c]) * d;
        }
        __syncthreads();
        {
            const int KG = m.m2 >> 3, tv = m.m1 >> 5;
            for (int t = wave; t < tv; t += NW) ev2g_ppo_back_tile<ACT>(E2, L.sB, KG, q.u2t + (size_t)t * KG * 256, t * 32, V1, L.sA, E1, L.sA);
        }
        __syncthreads();
        {
            const int kx = q.k1r >> 5, t4 = (m.m1 >> 5) * kx, t5 = (m.m2 >> 5) * (m.m1 >> 5);
            for (int t = wave; t < t4 + t5; t += NW) {
                int u = t;
                if (u < t4) { ev2g_ppo_dw_tile(E1, L.sA, (u / kx) * 32, X, L.sX, (u % kx) * 32, slab + q.slab_off[4], q.k1r, first); continue; }
                u -= t4;
                { const int kn = m.m1 >> 5; ev2g_ppo_dw_tile(E2, L.sB, (u / kn) * 32, V1, L.sA, (u % kn) * 32, slab + q.slab_off[6], m.m1, first); }
            }
            ev2g_ppo_colsum(E1, L.sA, m.m1, slab + q.slab_off[5], first);
            ev2g_ppo_colsum(E2, L.sB, m.m2, slab + q.slab_off[7], first);
            for (int c = threadIdx.x; c < m.m2; c += EV2G_PPO_BLOCK) {
                float *dst = slab + q.slab_off[10] + c;
                float s = first ? 0.0f : *dst;
                for (int r = 0; r < EV2G_PPO_ROWS; r++) s += g_v[r] * V2[r * L.sB + c];
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
    __syncthreads();
    double *sred = (double *)(base + L.oX);
    if ((threadIdx.x & 7) == 0) sred[threadIdx.x >> 3] = st0;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int r = 0; r < EV2G_PPO_ROWS; r++) s += sred[r];
        a.part[(size_t)blockIdx.x * 2] = s;
    }
}

__device__ __forceinline__ int ev2g_trpo_which(const TrpoMap &tm, int i) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < EV2G_TRPO_ACTOR_ARRAYS; j++) k += i >= tm.off[j] ? 1 : 0;
    return k;
}

// actor element i = the sum over the n_wg slabs, workgroups ascending, in float64.  fvp: the log_std block is 2 v (no slab), and every element
// gets damping v.  Else (the objective's gradient): the float32 rounding also goes into the thirteen-array gradient buffer, and block 0 writes
// J(theta0) = the partials' sum / B into the state.
template <typename T>
__global__ void __launch_bounds__(256) ev2g_trpo_reduce_kernel(PpoMap mp, TrpoMap tm, const float *__restrict__ work, int n_wg, int fvp, const T *__restrict__ v,
                                                             double damping, double *__restrict__ out64, float *__restrict__ out32, float *__restrict__ grad13,
                                                             const double *__restrict__ part, int B, TrpoState *st, int gate) {
    if (ev2g_trpo_gated(st, gate)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < tm.n_actor) {
        const int k = ev2g_trpo_which(tm, i), e = i - tm.off[k], arr = tm.arr[k];
        double s = 0.0;
        if (fvp && k == 0) s = 2.0 * (double)v[i];
        else {
            const int r = e / mp.cols[arr], c = e - r * mp.cols[arr];
            const float *src = work + mp.slab_off[arr] + (size_t)r * mp.slab_ld[arr] + c;
            for (int w = 0; w < n_wg; w++) s += (double)src[(size_t)w * mp.slab_floats];
        }
        if (fvp) s += damping * (double)v[i];
        if (out64) out64[i] = s;
        if (out32) out32[i] = (float)s;
        if (grad13) grad13[mp.off[arr] + e] = (float)s;
    }
    if (!fvp && blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < n_wg; w++) s += part[(size_t)w * 2];
        st->J0 = s / (double)B;
    }
}

// a flat actor vector into the direction images (the log_std block has none)
template <typename T>
__global__ void __launch_bounds__(256) ev2g_trpo_dir_kernel(TrpoMap tm, const T *__restrict__ v, const TrpoState *st, int gate) {
    if (ev2g_trpo_gated(st, gate)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tm.n_actor) return;
    const int k = ev2g_trpo_which(tm, i), e = i - tm.off[k];
    if (!tm.dimg[k]) return;
    const float t = (float)v[i];
    if (tm.img_k[k] == 0) { tm.dimg[k][e] = t; return; }
    const int r = e / tm.cols[k], c = e - r * tm.cols[k];
    tm.dimg[k][packed_f32_index(r, c, tm.img_k[k])] = t;
}

// a . b over n elements by the one workgroup: thread t's partial over elements t, t + 1024, ... then a fixed tree; every thread gets the sum
__device__ __forceinline__ double ev2g_trpo_dot(const double *__restrict__ a, const double *__restrict__ b, int n, double *red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += EV2G_TRPO_CG_BLOCK) s += a[i] * b[i];
    __syncthreads();   // (the previous dot's readers are done with red)
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = EV2G_TRPO_CG_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// x = 0, r = g, p = g rounded to float32, rho = g . g; the state of a new step.  p is kept float32-representable throughout: the product's
// direction images hold p itself, so H p is the product of the very p the dots and the updates of x and r use, and r = g - H x stays true to
// the product's own rounding (a float64 p whose float32 image goes through the product would break it by 2^-24 |H| |p| per iteration)
__global__ void __launch_bounds__(EV2G_TRPO_CG_BLOCK) ev2g_trpo_cg_init_kernel(int n, const double *__restrict__ g, double *__restrict__ x, double *__restrict__ r,
                                                                             double *__restrict__ p, TrpoState *st) {
    __shared__ double red[EV2G_TRPO_CG_BLOCK];
    for (int i = threadIdx.x; i < n; i += EV2G_TRPO_CG_BLOCK) { const double gi = g[i]; x[i] = 0.0; r[i] = gi; p[i] = (double)(float)gi; }
    const double rho = ev2g_trpo_dot(g, g, n, red);
    if (threadIdx.x == 0) {
        st->cg_done = rho < EV2G_TRPO_RHO_MIN ? 1 : 0; st->cg_iters = 0; st->ls_done = 0; st->ls_tries = 0; st->accepted = 0; st->failed = 0;
        st->rho = rho; st->J1 = 0.0; st->kl = 0.0; st->beta = 0.0; st->c = 1.0; st->xHx = 0.0;
    }
}

// one iteration from Hp (trpo_host_cg_step is its host twin)
__global__ void __launch_bounds__(EV2G_TRPO_CG_BLOCK) ev2g_trpo_cg_step_kernel(int n, const double *__restrict__ hp, double *__restrict__ x, double *__restrict__ r,
                                                                             double *__restrict__ p, TrpoState *st, int last) {
    __shared__ double red[EV2G_TRPO_CG_BLOCK];
    if (st->cg_done) return;   // (only thread 0 writes the state, after the last barrier)
    const double rho = st->rho;
    const double alpha = rho / ev2g_trpo_dot(p, hp, n, red);
    for (int i = threadIdx.x; i < n; i += EV2G_TRPO_CG_BLOCK) x[i] += alpha * p[i];
    if (last) {
        if (threadIdx.x == 0) { st->cg_iters += 1; st->cg_done = 1; }
        return;
    }
    for (int i = threadIdx.x; i < n; i += EV2G_TRPO_CG_BLOCK) r[i] -= alpha * hp[i];
    const double rn = ev2g_trpo_dot(r, r, n, red);
    const bool done = rn < EV2G_TRPO_RHO_MIN;
    if (!done) {
        const double b = rn / rho;
        for (int i = threadIdx.x; i < n; i += EV2G_TRPO_CG_BLOCK) p[i] = (double)(float)(r[i] + b * p[i]);
    }
    if (threadIdx.x == 0) { st->cg_iters += 1; st->rho = rn; if (done) st->cg_done = 1; }
}

// beta = sqrt(2 target_kl / (x . Hx)) from hx = H x; keeps theta0; a non-finite or non-positive x . Hx fails the step (no try is made)
__global__ void __launch_bounds__(EV2G_TRPO_CG_BLOCK) ev2g_trpo_stepsize_kernel(PpoMap mp, TrpoMap tm, const double *__restrict__ x, const double *__restrict__ hx,
                                                                              double target_kl, const float *__restrict__ theta, float *__restrict__ theta0,
                                                                              TrpoState *st) {
    __shared__ double red[EV2G_TRPO_CG_BLOCK];
    const int n = tm.n_actor;
    for (int i = threadIdx.x; i < n; i += EV2G_TRPO_CG_BLOCK) {
        const int k = ev2g_trpo_which(tm, i);
        theta0[i] = theta[mp.off[tm.arr[k]] + i - tm.off[k]];
    }
    const double xhx = ev2g_trpo_dot(x, hx, n, red);
    if (threadIdx.x == 0) {
        const bool ok = isfinite(xhx) && xhx > 0.0;
        st->xHx = xhx; st->beta = ok ? sqrt(2.0 * target_kl / xhx) : 0.0;
        st->failed = ok ? 0 : 1; st->ls_done = ok ? 0 : 1; st->c = 1.0;
    }
}

// theta = theta0 + c beta x into the masters and their places in the images
__global__ void __launch_bounds__(256) ev2g_trpo_candidate_kernel(PpoMap mp, TrpoMap tm, const double *__restrict__ x, const float *__restrict__ theta0,
                                                                float *__restrict__ theta, const TrpoState *st) {
    if (st->ls_done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tm.n_actor) return;
    const int k = ev2g_trpo_which(tm, i), ti = mp.off[tm.arr[k]] + i - tm.off[k];
    const float t = (float)((double)theta0[i] + (st->c * st->beta) * x[i]);
    theta[ti] = t;
    ev2g_ppo_place(mp, ti, t);
}

// one try's verdict from the evaluation's partials: accept if KL < target_kl and J > J(theta0), else shrink c; after the last failed try the
// masters and the images get theta0 back
__global__ void __launch_bounds__(EV2G_TRPO_CG_BLOCK) ev2g_trpo_decide_kernel(PpoMap mp, TrpoMap tm, const double *__restrict__ part, int n_wg, int B, double target_kl,
                                                                            double shrink, int last, const float *__restrict__ theta0, float *__restrict__ theta,
                                                                            TrpoState *st) {
    __shared__ int restore;
    if (st->ls_done) return;   // (only thread 0 writes the state, after the barrier)
    __syncthreads();
    if (threadIdx.x == 0) {
        double sj = 0.0, sk = 0.0;
        for (int w = 0; w < n_wg; w++) { sj += part[(size_t)w * 2]; sk += part[(size_t)w * 2 + 1]; }
        const double J = sj / (double)B, KL = sk / (double)B;
        const bool ok = KL < target_kl && J > st->J0;
        st->ls_tries += 1; st->J1 = J; st->kl = KL;
        if (ok) { st->accepted = 1; st->ls_done = 1; }
        else if (last) st->ls_done = 1;
        else st->c *= shrink;
        restore = (!ok && last) ? 1 : 0;
    }
    __syncthreads();
    if (!restore) return;
    for (int i = threadIdx.x; i < tm.n_actor; i += EV2G_TRPO_CG_BLOCK) {
        const int k = ev2g_trpo_which(tm, i), ti = mp.off[tm.arr[k]] + i - tm.off[k];
        const float t = theta0[i];
        theta[ti] = t;
        ev2g_ppo_place(mp, ti, t);
    }
}

__device__ __forceinline__ bool ev2g_trpo_is_value(int arr) { return (arr >= 4 && arr <= 7) || arr == 10 || arr == 11; }

// the six value arrays' gradient from the slabs (the actor's entries of the gradient buffer are left alone); block 0 writes value_loss
__global__ void __launch_bounds__(256) ev2g_trpo_vreduce_kernel(PpoMap mp, const float *__restrict__ work, const double *__restrict__ part, int n_wg, int B,
                                                              float *__restrict__ grad, float *__restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < mp.n_params) {
        const int arr = ev2g_ppo_which(mp, i);
        if (ev2g_trpo_is_value(arr)) {
            const int e = i - mp.off[arr], r = e / mp.cols[arr], c = e - r * mp.cols[arr];
            const float *src = work + mp.slab_off[arr] + (size_t)r * mp.slab_ld[arr] + c;
            double s = 0.0;
            for (int w = 0; w < n_wg; w++) s += (double)src[(size_t)w * mp.slab_floats];
            grad[i] = (float)s;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && stats) {
        double s = 0.0;
        for (int w = 0; w < n_wg; w++) s += part[(size_t)w * 2];
        stats[0] = (float)(s / (double)B);
    }
}

// Adam on the six value arrays and their places in the images; no clip
__global__ void __launch_bounds__(256) ev2g_trpo_vapply_kernel(PpoMap mp, const float *__restrict__ grad, AdamStep adam, float *__restrict__ theta,
                                                             float *__restrict__ am, float *__restrict__ av) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= mp.n_params || !ev2g_trpo_is_value(ev2g_ppo_which(mp, i))) return;
    float t = theta[i], mm = am[i], vv = av[i];
    ev2g_adam_elem(&t, &mm, &vv, grad[i], adam);
    theta[i] = t; am[i] = mm; av[i] = vv;
    ev2g_ppo_place(mp, i, t);
}
#endif
