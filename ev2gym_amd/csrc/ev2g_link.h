// ev2g_link.h -- the reference's two communication-fault models (ev2gym/rl_agent/noise_wrappers.py) applied on the device, before and after
// a one-step launch of the step kernel (the pattern of ev2g_heuristic.h: no step kernel changes).
//   ev2g_link_act_kernel<IN32>  FailedActionCommunication.action (noise_wrappers.py:37-60): one lane per (env, port).  A charger whose
//           uniform of this step is below p_fail keeps executing the command it was last sent; the delivered command is written into the
//           link's [E, P] block, which is both the wrapper's previous_actions_list and the action block the step kernel then reads (the step
//           kernels never modify the caller's actions, so the held value is what was SENT, as in the reference, which copies before the env
//           zeroes empty ports' entries, ev_charger.py:139).  IN32: float32 actions, widened as the engine widens them on entry.
//   ev2g_link_obs_kernel        DelayedObservation.observation, PublicPST branch (noise_wrappers.py:165-175,193-194): one wavefront per env,
//           ports in 64-slot chunks.  An occupied slot whose uniform is below p_delay shows the energy column DELIVERED one step earlier; the
//           energy that was not communicated is the difference of the raw column to the raw column of the step before, summed over the delayed
//           slots IN SLOT ORDER from 0 (a plain left-to-right float64 sum: the lanes' differences are read one by one, lowest slot first, the
//           idiom of ev2g_heuristic.h kinds 4 and 5; a tree sum gives other bits), and obs[2] -= (nc * 60) / timescale, clamped at 0 LAST.
//           Only column 4 + 3 i of the wrapper's two remembered rows is ever read: the state is two [E, P] arrays.
//           At the terminal observation (t == T) the reference indexes its [P, T] matrix out of range; here no slot is delayed there.
// Uniforms (LinkRand): a supplied matrix, stored [T, E, P] so that a step reads contiguously, or the engine's counter-based generator
// evaluated at index (e * P + i) * T + t under the link's seed -- the bits ev2g_host_uniform(n = E * P * T, seed, 0, 1) puts at [e, i, t].
// Every expression keeps the reference's operation order (-ffp-contract=off).
#pragma once
#include "ev2g_heuristic.h"

#define EV2G_LINK_BLOCK 256

struct LinkRand {
    const double *mat;         // [T, E, P], or nullptr: generated
    unsigned long long seed;
    int E, P, T;
};

__device__ __forceinline__ double ev2g_link_uniform(const LinkRand &r, int e, int i, int t) {
    if (r.mat) return r.mat[((long long)t * r.E + e) * r.P + i];
    return ev2g_u01(r.seed, (uint64_t)(((long long)e * r.P + i) * r.T + t));
}

template <bool IN32>
__global__ void __launch_bounds__(EV2G_LINK_BLOCK) ev2g_link_act_kernel(const void *in, LinkRand r, double p_fail, int t, double *__restrict__ held,
                                                                        double *out) {   // (out may be `in`: a block rewritten in place)
    const long long n = (long long)r.E * r.P;
    for (long long i = (long long)blockIdx.x * EV2G_LINK_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * EV2G_LINK_BLOCK) {
        const int e = (int)(i / r.P), p = (int)(i - (long long)e * r.P);
        const double a = IN32 ? (double)((const float *)in)[i] : ((const double *)in)[i];
        // np.where(random[:, step] < p_fail, previous, action); p_fail = 0 (ev2g_link_rollout's widening pass) holds nothing: no uniform drawn
        const double d = (p_fail > 0.0 && ev2g_link_uniform(r, e, p, t) < p_fail) ? held[i] : a;
        held[i] = d;
        if (out) out[i] = d;
    }
}

__global__ void __launch_bounds__(EV2G_LINK_BLOCK) ev2g_link_obs_kernel(double *__restrict__ obs, float *__restrict__ obs32, LinkRand r,
                                                                        double p_delay, int D, int t, double timescale,
                                                                        double *__restrict__ prev, double *__restrict__ actual) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * (EV2G_LINK_BLOCK >> 6) + wave;
    if (e >= r.E) return;
    const int P = r.P;
    double *o = obs + (long long)e * D;
    float *o32 = obs32 ? obs32 + (long long)e * D : nullptr;
    double *pv = prev + (long long)e * P, *av = actual + (long long)e * P;
    const bool live = t < r.T;   // the terminal observation passes through
    double nc = 0.0;             // not_communicated_energy_usage
    for (int base = 0; base < P; base += 64) {
        const int i = base + lane;
        const bool in = i < P;
        const double occ = in ? o[3 + 3 * i] : 0.0, en = in ? o[4 + 3 * i] : 0.0;
        const bool del = in && live && occ != 0.0 && ev2g_link_uniform(r, e, i, t) < p_delay;
        const double diff = del ? en - av[i] : 0.0;   // observation[4+3i] - actual_previous[4+3i]
        const double shown = del ? pv[i] : en;
        for (unsigned long long m = __ballot(del); m; m &= m - 1) nc += ev2g_lane_value(diff, __builtin_ctzll(m));
        if (in) {
            if (del) o[4 + 3 * i] = shown;
            pv[i] = shown;
            av[i] = en;
            if (o32) {
                o32[3 + 3 * i] = (float)occ;
                o32[4 + 3 * i] = (float)shown;
                o32[5 + 3 * i] = (float)o[5 + 3 * i];
            }
        }
    }
    if (lane == 0) {
        const double v = o[2] - nc * 60.0 / timescale;
        const double c = (v > 0.0) ? v : 0.0;   // max(0, v): the first argument unless the second is larger
        o[2] = c;
        if (o32) { o32[0] = (float)o[0]; o32[1] = (float)o[1]; o32[2] = (float)c; }
    }
}

// float32 copy of a float64 block (the policy's input row of ev2g_link_rollout when the link delays nothing)
__global__ void __launch_bounds__(EV2G_LINK_BLOCK) ev2g_link_f32_kernel(const double *__restrict__ src, float *__restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * EV2G_LINK_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * EV2G_LINK_BLOCK) dst[i] = (float)src[i];
}
