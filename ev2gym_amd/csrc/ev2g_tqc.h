// ev2g_tqc.h -- the distributional part of sb3_contrib's TQC.train() (Truncated Quantile Critics; MlpPolicy, Box actions, use_sde off) on the
// device.  Everything else of a TQC update is SAC's (ev2g_sac.h) and TD3's (ev2g_td3.h): the actor IS SAC's squashed Gaussian, the critics are the
// same three-layer ReLU networks through ev2g_td3_gemm_kernel with nq = n_quantiles outputs in place of one.
//
//   nc critics of nq quantiles each;  M = nc nq pooled atoms;  d atoms dropped per net;  K = M - d nc kept target atoms;  tau_i = (i + 0.5) / nq
//   target   per row b: the M atoms critic_target_j(s', a')[i], pooled j-major, sorted ascending, the first K kept:
//            z_k = r + ((1 - done) gamma) (sorted_k - alpha log pi')                                           (no gradient through z)
//   critics  delta = z_k - q_{j,i};  huber = |delta| - 0.5 where |delta| > 1, else 0.5 delta^2
//            critic_loss = mean over (b, j, i, k) of |tau_i - 1[delta < 0]| huber(delta)                        (one plain mean: B nc nq K terms)
//            d loss / d q_{j,i} = -(1 / (B nc nq K)) sum_k |tau_i - 1[delta < 0]| clamp(delta, -1, 1)
//   actor    actor_loss = mean_b(alpha log pi_b - mean_{j,i} critic_j(s, a_pi)[i]): every critic output's delta is 1 / (nc nq), the nc input
//            deltas are summed (j ascending) into g = d mean_{j,i} q / d a, and SAC's head backward applies the sign and the 1 / B
//
// THE SORT is a fixed compare-exchange network: the bitonic network of 128 keys, one wavefront per row, lane t one compare-exchange per stage, the
// keys in LDS.  A key is (value, pool index): equal values -- +0 and -0 among them -- keep their pool order, so the result is that of a stable
// sort under `<` and does not depend on anything but the row.  Slots past M hold (+inf, slot): they sort behind every atom (an atom that is +inf
// has a smaller index) and are never written out, K <= M.  LDS: a 32-lane half's `lo` (and `hi`) slots of a stage span 64 dwords while the
// partners are j < 32 apart -- two lanes per bank of the 32 that 4-byte reads and writes use, a two-way conflict on 25 of the 28 stages -- and
// are 32 consecutive dwords from j = 32 on, conflict-free.  A row is 28 stages of four reads and up to four writes per lane: of no weight next
// to the launch itself, so the keys are not swizzled.
//
// Every z, dq and loss element is formed in float64 from float32 operands in ONE fixed order (k ascending inside a (j, i) chain, the chains of a
// row joined m = j nq + i ascending, the rows by ev2g_td3_block_sum) and rounded once; no float atomics, no workgroup waits on another: the same
// call on the same state gives the same bits.  The element functions below are shared with the host twins (ev2g_tqc_host.h).
#pragma once
#include <stdint.h>
#include <math.h>

#define EV2G_TQC_MAX_CRITICS 5
#define EV2G_TQC_MAX_QUANTILES 64
#define EV2G_TQC_MAX_ATOMS 128     // the sorting network's width: two keys per lane of one wavefront
#define EV2G_TQC_ROWS 4            // batch rows (wavefronts) per workgroup of the two row kernels

// ---- element functions shared with the host twins (a host program defines __host__ and __device__ to nothing) ----
// the sort's order: by value, equal values (and +0 / -0) by pool index
__host__ __device__ inline bool ev2g_tqc_key_less(float va, int ia, float vb, int ib) { return va < vb || (!(vb < va) && ia < ib); }
__host__ __device__ inline double ev2g_tqc_tau(int i, int nq) { return ((double)i + 0.5) / (double)nq; }
// one (target atom z, current quantile q) pair under tau: its term of sum_k w clamp(delta, -1, 1) added to *g, its loss term to *l
__host__ __device__ inline void ev2g_tqc_pair(float z, float q, double tau, double *g, double *l) {
    const double d = (double)z - (double)q, w = d < 0.0 ? 1.0 - tau : tau, ad = fabs(d);
    *g += w * (d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d));
    *l += w * (ad > 1.0 ? ad - 0.5 : 0.5 * (d * d));
}
// 1 / (B nc nq K): the plain mean's weight
__host__ __device__ inline double ev2g_tqc_inv_terms(int B, int nc, int nq, int K) { return 1.0 / ((double)B * (double)nc * (double)nq * (double)K); }
// dq of one chain's sum g
__host__ __device__ inline float ev2g_tqc_dq_elem(double g, double inv_terms) { return (float)(-(g * inv_terms)); }

#ifdef __HIPCC__
// z [B, K] from the target critics' atoms tq [nc][B, nq] and log pi' [B]: one wavefront per row, EV2G_TQC_ROWS rows per workgroup.
__global__ void __launch_bounds__(64 * EV2G_TQC_ROWS) ev2g_tqc_target_kernel(const float *__restrict__ tq, const float *__restrict__ lp,
                                                                             const float *__restrict__ reward, const uint8_t *__restrict__ done, int B, int nc,
                                                                             int nq, int K, double gamma, const float *__restrict__ log_alpha,
                                                                             float *__restrict__ z) {
    __shared__ float key_v[EV2G_TQC_ROWS][EV2G_TQC_MAX_ATOMS];
    __shared__ int key_i[EV2G_TQC_ROWS][EV2G_TQC_MAX_ATOMS];
    const int w = threadIdx.x >> 6, t = threadIdx.x & 63, row = blockIdx.x * EV2G_TQC_ROWS + w, M = nc * nq;
    const bool live = row < B;
    float *kv = key_v[w];
    int *ki = key_i[w];
    for (int m = t; m < EV2G_TQC_MAX_ATOMS; m += 64) {   // lane order = pool order: atom m = j nq + i
        float v = INFINITY;
        if (live && m < M) { const int j = m / nq, i = m - j * nq; v = tq[((long long)j * B + row) * nq + i]; }
        kv[m] = v; ki[m] = m;
    }
    __syncthreads();
    for (int k = 2; k <= EV2G_TQC_MAX_ATOMS; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;   // lane t's pair of this stage: lo < hi < 128
            const float vl = kv[lo], vh = kv[hi];
            const int il = ki[lo], ih = ki[hi];
            const bool up = (lo & k) == 0;                                       // this stretch ascends
            if (ev2g_tqc_key_less(vh, ih, vl, il) == up) { kv[lo] = vh; ki[lo] = ih; kv[hi] = vl; ki[hi] = il; }
            __syncthreads();
        }
    if (!live) return;
    const double alpha = ev2g_sac_alpha(*log_alpha);
    const float r = reward[row], l = lp[row];
    const uint8_t dn = done[row];
    for (int k = t; k < K; k += 64) z[(long long)row * K + k] = ev2g_sac_y_elem(r, dn, gamma, kv[k], alpha, l);
}

// dq [nc][B, nq] and the row's loss partial part[B] (float64: the row's sum of w huber over (j, i, k)) from z [B, K] and q [nc][B, nq]: one
// wavefront per row, lane t the chains m = t and t + 64, each over k ascending; lane 0 joins the row's M chain losses m ascending.
__global__ void __launch_bounds__(64 * EV2G_TQC_ROWS) ev2g_tqc_critic_head_kernel(const float *__restrict__ z, const float *__restrict__ q, int B, int nc, int nq,
                                                                                  int K, float *__restrict__ dq, double *__restrict__ part) {
    __shared__ float zs[EV2G_TQC_ROWS][EV2G_TQC_MAX_ATOMS];
    __shared__ double ls[EV2G_TQC_ROWS][EV2G_TQC_MAX_ATOMS];
    const int w = threadIdx.x >> 6, t = threadIdx.x & 63, row = blockIdx.x * EV2G_TQC_ROWS + w, M = nc * nq;
    const bool live = row < B;
    const double inv_terms = ev2g_tqc_inv_terms(B, nc, nq, K);
    if (live)
        for (int k = t; k < K; k += 64) zs[w][k] = z[(long long)row * K + k];
    __syncthreads();
    if (live)
        for (int m = t; m < M; m += 64) {
            const int j = m / nq, i = m - j * nq;
            const long long at = ((long long)j * B + row) * nq + i;
            const float qv = q[at];
            const double tau = ev2g_tqc_tau(i, nq);
            double g = 0.0, l = 0.0;
            for (int k = 0; k < K; k++) ev2g_tqc_pair(zs[w][k], qv, tau, &g, &l);
            dq[at] = ev2g_tqc_dq_elem(g, inv_terms);
            ls[w][m] = l;
        }
    __syncthreads();
    if (live && t == 0) {
        double s = 0.0;
        for (int m = 0; m < M; m++) s += ls[w][m];
        part[row] = s;
    }
}

// losses[0] = critic_loss: the rows' partials joined in ev2g_td3_block_sum's order, times 1 / (B nc nq K).  One workgroup.
__global__ void __launch_bounds__(256) ev2g_tqc_loss_join_kernel(const double *__restrict__ part, int B, int nc, int nq, int K, float *__restrict__ losses) {
    __shared__ double red[256];
    const double s = ev2g_td3_block_sum(B, red, [&](int b) { return part[b]; });
    if (threadIdx.x == 0) losses[0] = (float)(s * ev2g_tqc_inv_terms(B, nc, nq, K));
}

// The actor's head on q [nc][B, nq] = critic_j(s, a_pi) and log pi [B]: part[b] = the row's sum of its M atoms (m ascending, float64) -- one thread
// per row, grid-strided -- and dq [nc][B, nq] = 1 / (nc nq), the output delta of mean_{j,i} q.
__global__ void __launch_bounds__(256) ev2g_tqc_actor_rows_kernel(const float *__restrict__ q, int B, int nc, int nq, float *__restrict__ dq, double *__restrict__ part) {
    const float d = (float)(1.0 / ((double)nc * (double)nq));
    const long long n = (long long)nc * B * nq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dq[i] = d;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nq; i++) s += (double)q[((long long)j * B + b) * nq + i];
        part[b] = s;
    }
}
// losses[1] = actor_loss = mean_b(alpha log pi_b - part_b / (nc nq)), [2] = ent_coef_loss, [3] = alpha; g_alpha = -mean(log pi + target_entropy)
// (fixed coefficient: 0) -- SAC's conventions (ev2g_sac_actor_head_kernel).  One workgroup.
__global__ void __launch_bounds__(256) ev2g_tqc_actor_head_kernel(const double *__restrict__ part, const float *__restrict__ lp, int B, int nc, int nq,
                                                                  const float *__restrict__ log_alpha, double target_entropy, int auto_alpha,
                                                                  float *__restrict__ losses, float *__restrict__ g_alpha) {
    const double inv_b = 1.0 / (double)B, la = (double)*log_alpha, alpha = ev2g_sac_alpha(*log_alpha), inv_m = 1.0 / ((double)nc * (double)nq);
    __shared__ double red[256];
    const double s1 = ev2g_td3_block_sum(B, red, [&](int b) { return alpha * (double)lp[b] - part[b] * inv_m; });
    const double s2 = ev2g_td3_block_sum(B, red, [&](int b) { return (double)lp[b] + target_entropy; });
    if (threadIdx.x == 0) {
        const double g = -(s2 * inv_b);
        losses[1] = (float)(s1 * inv_b);
        losses[2] = auto_alpha ? (float)(la * g) : 0.0f;
        losses[3] = (float)alpha;
        *g_alpha = auto_alpha ? (float)g : 0.0f;
    }
}

// out [n] = sum_j dxa[j][n], j ascending, float64 rounded once: the critics' input deltas [nc][B, P] into g = d mean_{j,i} q / d a
__global__ void ev2g_tqc_delta_sum_kernel(const float *__restrict__ dxa, int nc, long long n, float *__restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        double s = (double)dxa[i];
        for (int j = 1; j < nc; j++) s += (double)dxa[(long long)j * n + i];
        out[i] = (float)s;
    }
}
#endif
