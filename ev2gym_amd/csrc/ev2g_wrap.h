// ev2g_wrap.h -- the reference's gym action wrappers (ev2gym/rl_agent/action_wrappers.py) applied on the device, ahead of a one-step launch of
// the step kernel (the pattern of ev2g_heuristic.h / ev2g_link.h: no step kernel changes).
//   ev2g_wrap_discrete_kernel<IN32>  BinaryAction.action (action_wrappers.py:47) and ThreeStep_Action.action / ThreeStep_Action_DiscreteActionSpace
//           .action (:90, :138, the same body): one lane per (env, port), any number of ports per charger.
//           min_action[p] = cs_min_charge_current / cs_max_charge_current + 1e-4 of the port's charger.
//   ev2g_wrap_repair_kernel<IN32>    Rescale_RepairLayer.action (:277-451): one wavefront per env.  The wrapper's ev_buffer (port ids) with every
//           entry's min_power / max_power lives in WrapArgs::queue / qmin / qmax between calls and is staged in LDS with the proposed powers;
//           the queue passes are those of ev2g_heuristic.h kinds 4 and 5 (insert at the front in ascending port order, keep the powers an
//           entry was INSERTED with, compact in order), written anew here so that the heuristic kernels compile as they did.  Unlike the agents'
//           queue this one is NOT emptied at step 0: the reference's wrapper object lives across reset().
//           Every sum is the plain left-to-right float64 sum from 0 in queue order (Python's sum() before CPython 3.12, and the wrapper's own
//           `+=` loop): the wavefront reads 64 entries at a time and every lane adds them one by one, lane 0's first.  A tree sum flips the
//           branch comparisons.  The greedy top-up of the reduction branch (:413-421) is a dependent loop run the same way.
//           Two quirks of the reference are reproduced: a port whose next EV arrives the step after the last one left keeps the old EV's
//           powers, and new_action[i] = proposed[i] / max_cs_power[i] divides by the charger at the QUEUE POSITION i, not by the port's own
//           (:356, :429).  One port per charger only (:186): port p is charger p.
//           Port limit: one env's stage (three float64 lists, the port ids and a flag byte per port: 29 bytes per port, 16-byte aligned) has
//           to fit the 64 KiB of LDS -- EV2G_WRAP_MAX_PORTS = 2259.
// IN32: the input row is float32, widened to float64 first, as the engine widens float32 actions.  `out` may be `in` (a float64 block rewritten
// in place): every element is read before it is written, by the lane that writes it or ahead of a wavefront barrier.
// Every expression keeps the reference's operation order (-ffp-contract=off).
#pragma once
#include "ev2g_heuristic.h"

#define EV2G_WRAP_BLOCK 256
#define EV2G_WRAP_KIND_BINARY 0
#define EV2G_WRAP_KIND_THREE_STEP 1
#define EV2G_WRAP_MAX_PORTS 2259

struct WrapArgs {
    const int *port_slot;      // [P] slot of every reference port
    const double *cs_kw;       // [C] EV_Charger.get_max_power, the reference's operation order (HeurArgs::cs_kw)
    const double *cs_min_kw;   // [C] EV_Charger.get_min_charge_power
    int *queue, *qlen;         // [E, P], [E] Rescale_RepairLayer.ev_buffer of every env
    double *qmin, *qmax;       // [E, P] its min_power / max_power lists, entry for entry next to `queue`
    int scn_off;               // env e runs scenario (e + scn_off) mod M
};

// LDS bytes of one env's repair stage: min_power, max_power and proposed_power (double [P] each), the new queue (int [P]), a flag byte per port
__host__ __device__ inline size_t ev2g_wrap_wave_bytes(int P) { return ((size_t)P * 24 + (size_t)P * 4 + (size_t)P + 15) & ~(size_t)15; }

// min_action of reference port p: cs.min_charge_current / cs.max_charge_current + epsilon of its charger (action_wrappers.py:31-32, :190-191)
__device__ __forceinline__ double ev2g_wrap_min_action(const DevScn &s, const int *port_slot, int p) {
    const int cs = s.slot_cs[port_slot[p]];
    return s.cs_imin[cs] / s.cs_imax[cs] + 1e-4;
}

__device__ __forceinline__ double ev2g_wrap_in(const void *in, long long i, bool in32) {
    return in32 ? (double)((const float *)in)[i] : ((const double *)in)[i];
}

// np.clip(x, lo, hi) = minimum(maximum(x, lo), hi); a NaN x stays NaN
__device__ __forceinline__ double ev2g_wrap_clip(double x, double lo, double hi) {
    const double m = (x < lo) ? lo : x;
    return (m > hi) ? hi : m;
}

// the plain left-to-right float64 sum of f(0) .. f(n - 1), the same in every lane
template <typename F>
__device__ __forceinline__ double ev2g_wrap_sum(int n, int lane, F f) {
    double total = 0.0;
    for (int base = 0; base < n; base += 64) {
        const double v = (base + lane < n) ? f(base + lane) : 0.0;
        const int cnt = min(64, n - base);
        for (int j = 0; j < cnt; j++) total += ev2g_lane_value(v, j);
    }
    return total;
}

template <bool IN32>
__global__ void __launch_bounds__(EV2G_WRAP_BLOCK) ev2g_wrap_discrete_kernel(DevScn s, const int *__restrict__ port_slot, int kind, const void *in,
                                                                             double *out) {   // (out may be `in`)
    const int P = s.P;
    const long long n = (long long)s.E * P;
    for (long long i = (long long)blockIdx.x * EV2G_WRAP_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * EV2G_WRAP_BLOCK) {
        const int p = (int)(i % P);
        const double a = ev2g_wrap_in(in, i, IN32), lo = ev2g_wrap_min_action(s, port_slot, p);
        double v;
        if (kind == EV2G_WRAP_KIND_BINARY) v = (a > 0.5) ? 1.0 : lo;          // np.where(action > 0.5, 1, min_action)
        else v = (a == 0.0) ? 0.0 : ((a == 1.0) ? lo : 1.0);                  // np.where(action == 0, 0, np.where(action == 1, min_action, 1))
        out[i] = v;
    }
}

template <bool IN32>
__global__ void __launch_bounds__(EV2G_WRAP_BLOCK) ev2g_wrap_repair_kernel(DevScn s, DevState st, WrapArgs a, int t, const void *in, double *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wrap_lds[];
    const int P = s.P;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * (blockDim.x >> 6) + wave;
    if (e >= s.E) return;
    unsigned char *stage = wrap_lds + (size_t)wave * ev2g_wrap_wave_bytes(P);
    double *nmin = (double *)stage, *nmax = nmin + P, *prop = nmax + P;   // the new queue's min_power / max_power, proposed_power
    int *nq = (int *)(prop + P);                                          // the new queue
    unsigned char *fl = (unsigned char *)(nq + P);                        // per port: 1 wants charge (= occupied_ports after the update), 2 in the old queue
    const long long row = (long long)e * P;
    int *q = a.queue + row;
    const int len = min(a.qlen[e], P);   // (kept across resets: the wrapper object outlives the episode)
    const HeurArgs ha{a.port_slot};
    for (int p = lane; p < P; p += 64) {   // :213-214: an EV is connected and get_soc() < 1
        int slot, t_dep;
        double cap;
        const int ss = ev2g_heur_port(s, st, ha, e, p, t, slot, cap, t_dep);
        fl[p] = (ss >= 0 && cap / s.ss_B[ss] < 1.0) ? 1 : 0;
    }
    ev2g_wave_sync();
    for (int i = lane; i < len; i += 64) {   // (a port id is queued at most once)
        const int p = q[i];
        if ((unsigned)p < (unsigned)P) fl[p] |= 2;
    }
    ev2g_wave_sync();
    // update_ev_buffer (:205-243): the ports that want charge and are not queued go to the front -- inserted at index 0 in ascending port
    // order, i.e. in descending order -- with the powers of the EV that is parked now ...
    int n = 0;
    for (int base = ((P - 1) >> 6) << 6; base >= 0; base -= 64) {
        const int p = base + lane;
        const bool add = p < P && (fl[p] & 3) == 1;
        const unsigned long long m = __ballot(add);
        if (add) {
            const int at = n + __popcll((m >> lane) >> 1);   // the lanes above this one come first
            int slot, t_dep;
            double cap;
            const int ss = ev2g_heur_port(s, st, ha, e, p, t, slot, cap, t_dep);
            const int cs = s.slot_cs[slot];
            const double cs_lo = a.cs_min_kw[cs], ev_lo = s.ss_pacmin[ss], cs_hi = a.cs_kw[cs], ev_hi = s.ss_pacmax[ss];
            nq[at] = p;
            nmin[at] = (ev_lo > cs_lo) ? ev_lo : cs_lo;   // max(charger, EV): the first argument unless the second is larger
            nmax[at] = (ev_hi < cs_hi) ? ev_hi : cs_hi;   // min(charger, EV)
        }
        n += __popcll(m);
    }
    // ... followed by the queued ports that still want charge, in their order and with the powers they were inserted with
    for (int base = 0; base < len; base += 64) {
        const int i = base + lane;
        const int p = (i < len) ? q[i] : -1;
        const bool keep = (unsigned)p < (unsigned)P && (fl[p] & 1);
        const unsigned long long m = __ballot(keep);
        const int at = n + ev2g_lanes_below(m);
        if (keep && at < P) {
            nq[at] = p;
            nmin[at] = a.qmin[row + i];
            nmax[at] = a.qmax[row + i];
        }
        n = min(n + __popcll(m), P);   // (the queue never holds more than P distinct ports; the bound only guards the stage)
    }
    ev2g_wave_sync();
    // :274, :325-326: the rescaled action's power, clamped to the entry's range (calculate_total_power computes the same values)
    for (int i = lane; i < n; i += 64) {
        const int p = nq[i];
        const double lo = ev2g_wrap_min_action(s, a.port_slot, p);
        const double r = ev2g_wrap_in(in, row + p, IN32) * (1.0 - lo) + lo;
        prop[i] = ev2g_wrap_clip(r * a.cs_kw[p], nmin[i], nmax[i]);
    }
    ev2g_wave_sync();
    const double current = ev2g_wrap_sum(n, lane, [&](int i) { return prop[i]; });
    const double sp = s.setpoint[(long long)ev2g_scn(e, a.scn_off, s.M) * s.T + t];
    const bool raise = current < sp, reduce = !raise && current > sp;
    if (raise) {   // :312-371
        const double deficit = sp - current;
        const double range = ev2g_wrap_sum(n, lane, [&](int i) { return nmax[i] - prop[i]; });
        if (range > 0.0) {
            const double x = deficit / range, f = (x < 1.0) ? x : 1.0;   // min(1, x)
            for (int i = lane; i < n; i += 64) {
                const double hi = nmax[i], v = prop[i] + (hi - prop[i]) * f;
                prop[i] = (hi < v) ? hi : v;   // min(new_power, max_power)
            }
        }
    } else if (reduce) {   // :373-444
        const double excess = current - sp;
        const double range = ev2g_wrap_sum(n, lane, [&](int i) { return prop[i] - nmin[i]; });
        if (range > 0.0) {
            const double x = excess / range, f = (x < 1.0) ? x : 1.0;
            for (int i = lane; i < n; i += 64) {
                const double lo = nmin[i], v = prop[i] - (prop[i] - lo) * f;
                prop[i] = (lo > v) ? lo : v;   // max(new_power, min_power)
            }
            ev2g_wave_sync();
        }
        // rounding alone can leave the total below the setpoint: the greedy top-up, entry by entry in queue order, every lane alike
        double rem = sp - ev2g_wrap_sum(n, lane, [&](int i) { return prop[i]; });
        if (rem > 0.0) {
            bool more = true;
            for (int base = 0; base < n && more; base += 64) {
                const int i = base + lane;
                const double room = (i < n) ? nmax[i] - prop[i] : 0.0;
                double mine = 0.0;
                bool hit = false;
                const int cnt = min(64, n - base);
                for (int j = 0; j < cnt; j++) {
                    if (rem <= 0.0) { more = false; break; }
                    const double r = ev2g_lane_value(room, j), inc = (r < rem) ? r : rem;   // min(remaining_deficit, increaseable_amount)
                    if (lane == j) { mine = inc; hit = true; }
                    rem -= inc;
                }
                if (hit) prop[i] += mine;
            }
        }
    }
    ev2g_wave_sync();
    // :371 / :444 / :451: action * occupied_ports -- a multiplication, so that a negative rescaled action on an unqueued port gives the
    // reference's zero; in the two adjusting branches the queued ports take proposed_power / max_cs_power of their QUEUE POSITION
    const bool adjust = raise || reduce;
    for (int p = lane; p < P; p += 64) {
        const bool occ = fl[p] & 1;
        if (occ && adjust) continue;
        const double lo = ev2g_wrap_min_action(s, a.port_slot, p);
        const double r = ev2g_wrap_in(in, row + p, IN32) * (1.0 - lo) + lo;
        out[row + p] = r * (occ ? 1.0 : 0.0);
    }
    for (int i = lane; i < n; i += 64) {
        if (adjust) out[row + nq[i]] = prop[i] / a.cs_kw[i] * 1.0;
        q[i] = nq[i];
        a.qmin[row + i] = nmin[i];
        a.qmax[row + i] = nmax[i];
    }
    if (lane == 0) a.qlen[e] = n;
}
