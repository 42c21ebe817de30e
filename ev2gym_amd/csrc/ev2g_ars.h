// ev2g_ars.h -- sb3_contrib's ARS (Augmented Random Search) on the device: an iteration evaluates 2 n_delta perturbed copies of a deterministic
// policy for whole episodes and steps theta from the episode returns.  No backprop, no replay.  The layouts, the element functions and the
// host twins are ev2g_ars_host.h's.
//
// THE POPULATION ACTOR (ev2g_ars_act_kernel) is ev2g_ac.h's 32-row exact-f32 MFMA workgroup over pack_linear_f32 images with a CANDIDATE PER
// WORKGROUP: the n_rows = C R rows are C candidates of R consecutive rows, a candidate takes ceil(R / 32) workgroups, and workgroup b reads
// the images of candidate b / ceil(R / 32) at base + c * stride (ars_tile_of).  C = 1 over the centre image is the policy theta itself.
// MlpPolicy: ReLU trunk, linear head, tanhf, unscaled into [lo, 1]; LinearPolicy: one linear tile row, clipped to [lo, 1].  Every output
// element is one fixed k-ordered chain of its own row over its candidate's weights: it does not depend on R, C or the row's place.
//
// ev2g_ars_perturb_kernel draws the directions (no stored stream: ev2g_ac_normal at ars_delta_index) and writes w+- straight to their packed
// positions; ev2g_ars_returns_kernel adds kept reward rows to the envs' returns; ev2g_ars_candidates_kernel sums a candidate's envs;
// ev2g_ars_rank_kernel ranks, checks and forms the step in one workgroup; ev2g_ars_step_kernel moves theta and repacks the centre image.
// Sums run in one fixed order, no atomics.
#pragma once
#include "ev2g_ac.h"
#include "ev2g_ars_host.h"

template <int KIND>
__global__ void __launch_bounds__(EV2G_AC_BLOCK) ev2g_ars_act_kernel(ArsDev m, const float *__restrict__ images, const float *__restrict__ x, int R,
                                                                    float *__restrict__ act) {
    extern __shared__ __attribute__((aligned(16))) float ars_lds[];
    const ArsLds L = ev2g_ars_lds(m);
    float *bufA = ars_lds, *bufB = bufA + EV2G_AC_ROWS * L.sA;
    const int wave = threadIdx.x >> 6;
    const ArsTile tile = ars_tile_of((int)blockIdx.x, R);
    const float *img = images + (size_t)tile.cand * (size_t)m.stride;
    const long long row0 = tile.row0;
    const int nr = tile.live;
    // input rows -> LDS, zeros past the last live row and past D
    for (int i = threadIdx.x; i < EV2G_AC_ROWS * m.k1; i += EV2G_AC_BLOCK) {
        const int r = i / m.k1, c = i - r * m.k1;
        bufA[r * L.sA + c] = (r < nr && c < m.d_in) ? x[(size_t)(row0 + r) * m.d_in + c] : 0.0f;
    }
    __syncthreads();
    if (KIND == EV2G_ARS_MLP) {
        {   // A -> B
            const int KG = m.k1 >> 3;
            for (int t = wave; t < (m.n1 >> 5); t += EV2G_AC_BLOCK / 64)
                ev2g_ac_tile<EV2G_AC_RELU>(bufA, L.sA, KG, img + m.o_w1 + (size_t)t * KG * 256, img + m.o_b1, t * 32, bufB, L.sB);
        }
        __syncthreads();
        {   // B -> A
            const int KG = m.n1 >> 3;
            for (int t = wave; t < (m.n2 >> 5); t += EV2G_AC_BLOCK / 64)
                ev2g_ac_tile<EV2G_AC_RELU>(bufB, L.sB, KG, img + m.o_w2 + (size_t)t * KG * 256, img + m.o_b2, t * 32, bufA, L.sA);
        }
        __syncthreads();
    }
    {   // the head: A -> B, linear
        const int KG = (KIND == EV2G_ARS_MLP ? m.n2 : m.k1) >> 3;
        for (int t = wave; t < (m.n3 >> 5); t += EV2G_AC_BLOCK / 64)
            ev2g_ac_tile<EV2G_AC_LINEAR>(bufA, L.sA, KG, img + m.o_w3 + (size_t)t * KG * 256, img + m.o_b3, t * 32, bufB, L.sB);
    }
    __syncthreads();
    const int row = threadIdx.x >> 3, j = threadIdx.x & 7;
    if (row < nr)
        for (int p = j; p < m.d_out; p += 8) {
            const float v = bufB[row * L.sB + p];
            act[(size_t)(row0 + row) * m.d_out + p] = KIND == EV2G_ARS_MLP ? ev2g_sac_unscale_action(tanhf(v), m.lo) : fminf(fmaxf(v, m.lo), 1.0f);
        }
}

// delta [n_delta, n_params] of iteration n, and candidates k / n_delta + k of every element at its packed position in cand (2 n_delta images)
__global__ void ev2g_ars_perturb_kernel(const ArsLayout L, const float *__restrict__ theta, int n_delta, float std32, uint64_t seed, uint64_t n,
                                        long long stride, float *__restrict__ delta, float *__restrict__ cand) {
    const long long total = (long long)n_delta * L.n_params;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(q / L.n_params), i = (int)(q - (long long)k * L.n_params);
        const float d = ev2g_ac_normal(seed, ars_delta_index(n, n_delta, L.n_params, k, i));
        float wp, wm;
        ars_perturb_elem(theta[i], d, std32, &wp, &wm);
        delta[q] = d;
        const long long at = ars_image_index(L, i);
        cand[(long long)k * stride + at] = wp;
        cand[(long long)(n_delta + k) * stride + at] = wm;
    }
}

// env_return [E] += the kept rows reward [k, stride], t ascending per env
__global__ void ev2g_ars_returns_kernel(double *__restrict__ env_return, const double *__restrict__ reward, int k, long long stride, int E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) env_return[e] = ars_env_return(env_return[e], reward, k, stride, e);
}

// ret [C]: candidate c's R envs ascending, then the alive bonus
__global__ void ev2g_ars_candidates_kernel(const double *__restrict__ env_return, int R, int C, double alive_bonus_offset, long long steps,
                                           double *__restrict__ ret) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) ret[c] = ars_candidate_return(env_return, R, c, alive_bonus_offset, steps);
}

// One workgroup: rank [n_delta] by counting and order [rank] = k, then thread 0 checks the returns and forms sigma_R and the step serially
__global__ void __launch_bounds__(256) ev2g_ars_rank_kernel(const double *__restrict__ ret, int n_delta, int n_top, double lr, long long iteration,
                                                            int32_t *__restrict__ rank, int32_t *__restrict__ order, ev2g_ars_report *__restrict__ rep) {
    for (int k = threadIdx.x; k < n_delta; k += blockDim.x) {
        const int r = ars_rank_of(ret, n_delta, k);
        rank[k] = r; order[r] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int bad = ars_first_bad(ret, n_delta);
        double sigma = 0.0, step = 0.0;
        if (bad < 0) ars_step_of(ret, order, n_delta, n_top, lr, &sigma, &step);
        rep->sigma_r = sigma; rep->step = step; rep->iteration = iteration; rep->refused = bad >= 0 ? 1 : 0; rep->first_bad = bad; rep->n_top = n_top;
        rep->reserved = 0;
    }
}

// theta's step and the centre image's element, unless the update was refused
__global__ void ev2g_ars_step_kernel(const ArsLayout L, float *__restrict__ theta, const float *__restrict__ delta, const double *__restrict__ ret,
                                     const int32_t *__restrict__ order, const ev2g_ars_report *__restrict__ rep, int n_delta, int n_top,
                                     float *__restrict__ centre) {
    if (rep->refused) return;
    const double step = rep->step;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n_params; i += gridDim.x * blockDim.x) {
        const float v = ars_theta_elem(theta[i], ret, order, delta, n_delta, n_top, L.n_params, i, step);
        theta[i] = v;
        centre[ars_image_index(L, i)] = v;
    }
}

// the centre image from theta (create, ev2g_ars_set_weights)
__global__ void ev2g_ars_repack_kernel(const ArsLayout L, const float *__restrict__ theta, float *__restrict__ centre) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n_params; i += gridDim.x * blockDim.x) centre[ars_image_index(L, i)] = theta[i];
}
