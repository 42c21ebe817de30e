// ev2g_heuristic.h -- the reference's env-reading heuristic agents (ev2gym/baselines/heuristics.py) evaluated on the device state.
//
// One launch computes the actions [E, P] (reference port order) the agent would choose for the current step t, from the engine's
// persistent state as it stands before step t: every port's PortLine and the scenario arrays of DevScn.  Nothing is read from the
// host (after ev2g_pool_refill the host holds no copy of the scenarios).
//   kind 0  ChargeAsLateAsPossible                   heuristics.py:98-149   one lane per (env, port)
//   kind 1  ChargeAsFastAsPossibleToDesiredCapacity  heuristics.py:230-267  one lane per (env, port)
//   kind 2  RoundRobin                               heuristics.py:7-96     one wavefront per env: the agent's queue of port ids lives in
//           HeurArgs::queue between calls and is staged in LDS; every order-preserving pass is an in-order compaction (ballot + prefix count)
// A port holds an EV when its window covers t and its session list is not exhausted (ev2g_peek's port_session); that EV's
// current_capacity is the line's `cap`.  Every expression keeps the reference's operation order (-ffp-contract=off): a one-ulp
// difference flips a ceil or a `<` and with it an action.
#pragma once
#include "ev2g_device.h"

#define EV2G_HEUR_BLOCK 256
#define EV2G_HEUR_CALP 0
#define EV2G_HEUR_CAFTDC 1
#define EV2G_HEUR_RR 2

struct HeurArgs {
    const int *port_slot;   // [P] slot of every reference port
    const double *cs_kw;    // [C] max_charge_current * voltage * sqrt(phases) / 1000, in that order (EV_Charger.get_max_power)
    double avg_power;       // RoundRobin.average_power: sequential sum over chargers of I * V * sqrt(phases) / n_ports, divided by C
    int *queue;             // [E, P] RoundRobin's ev_buffer of every env (port ids, next to be served first)
    int *qlen;              // [E]
    int scn_off;            // env e runs scenario (e + scn_off) mod M
};

// LDS bytes of one env's RoundRobin stage: the new queue (int [P]) and a flag byte per port, 16-byte aligned
__host__ __device__ inline size_t ev2g_heur_rr_wave_bytes(int P) { return ((size_t)P * 4 + (size_t)P + 15) & ~(size_t)15; }

// orders this lane's LDS accesses against the other lanes of its wavefront (the wavefront runs in lockstep; this keeps the compiler
// from moving them across a phase boundary)
__device__ __forceinline__ void ev2g_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// number of lanes below this one whose bit is set in `mask`
__device__ __forceinline__ int ev2g_lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// the EV connected to reference port p of env e before step t: its session index, or -1 when the port is empty
__device__ __forceinline__ int ev2g_heur_port(const DevScn &s, const DevState &st, const HeurArgs &a, int e, int p, int t, int &slot,
                                              double &cap, int &t_dep) {
    slot = a.port_slot[p];
    const PortLine *l = st.line + (long long)e * s.P + slot;
    const int4 w = *(const int4 *)l;   // ta, td, ss, cyc_lut
    cap = l->cap;
    t_dep = w.y;
    return (w.x <= t && t <= w.y && w.z >= 0) ? w.z : -1;
}

template <int KIND>
__global__ void __launch_bounds__(EV2G_HEUR_BLOCK) ev2g_heuristic_kernel(DevScn s, DevState st, HeurArgs a, int t, double *__restrict__ actions) {
    const int P = s.P;
    if constexpr (KIND != EV2G_HEUR_RR) {
        const long long i = (long long)blockIdx.x * EV2G_HEUR_BLOCK + threadIdx.x;
        if (i >= (long long)s.E * P) return;
        const int e = (int)(i / P), p = (int)(i - (long long)e * P);
        int slot, t_dep;
        double cap;
        const int ss = ev2g_heur_port(s, st, a, e, p, t, slot, cap, t_dep);
        double v = 0.0;
        if (ss >= 0) {
            const double cs_kw = a.cs_kw[s.slot_cs[slot]], pac = s.ss_pacmax[ss], ts = (double)s.dt;
            const double pw = (pac < cs_kw) ? pac : cs_kw;   // min(charger, EV): the first argument unless the second is smaller
            if constexpr (KIND == EV2G_HEUR_CALP) {          // heuristics.py:119-131
                const double B = s.ss_B[ss];
                const double soc = cap / B;
                const double steps = ceil((1.0 - soc) / (pw * ts / 60.0 / B));
                if (soc < 1.0 && (double)t_dep - steps <= (double)t) v = 1.0;
            } else {                                         // heuristics.py:251-264
                const double des = s.ss_des[ss];
                if (cap + pw * ts / 60.0 < des) {
                    v = 1.0;
                } else {
                    const double x = (des - cap) * 60.0 / ts / cs_kw;
                    v = (0.0 > x) ? 0.0 : x;   // max(x, 0)
                }
            }
        }
        actions[i] = v;
    } else {
        extern __shared__ __attribute__((aligned(16))) unsigned char heur_lds[];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int e = blockIdx.x * (blockDim.x >> 6) + wave;
        if (e >= s.E) return;
        int *nq = (int *)(heur_lds + (size_t)wave * ev2g_heur_rr_wave_bytes(P));   // the new queue
        unsigned char *fl = (unsigned char *)(nq + P);   // per port: 1 wants charge, 2 in the old queue, 4 charges this step
        int *q = a.queue + (long long)e * P;
        const int len = (t == 0) ? 0 : min(a.qlen[e], P);   // every episode starts with a fresh agent (evaluator.py:237)
        for (int p = lane; p < P; p += 64) {             // wants charge: an EV is connected and not full
            int slot, t_dep;
            double cap;
            const int ss = ev2g_heur_port(s, st, a, e, p, t, slot, cap, t_dep);
            fl[p] = (ss >= 0 && cap / s.ss_B[ss] < 1.0) ? 1 : 0;
        }
        ev2g_wave_sync();
        for (int i = lane; i < len; i += 64) {   // (a port id is queued at most once)
            const int p = q[i];
            if ((unsigned)p < (unsigned)P) fl[p] |= 2;
        }
        ev2g_wave_sync();
        // update_ev_buffer (heuristics.py:33-52): the ports that want charge and are not queued go to the front -- inserted at index 0 in
        // ascending port order, i.e. in descending order ...
        int n = 0;
        for (int base = ((P - 1) >> 6) << 6; base >= 0; base -= 64) {
            const int p = base + lane;
            const bool add = p < P && (fl[p] & 3) == 1;
            const unsigned long long m = __ballot(add);
            if (add) nq[n + __popcll((m >> lane) >> 1)] = p;   // the lanes above this one come first
            n += __popcll(m);
        }
        // ... followed by the queued ports that still want charge, in their order (the others are removed)
        for (int base = 0; base < len; base += 64) {
            const int i = base + lane;
            const int p = (i < len) ? q[i] : -1;
            const bool keep = (unsigned)p < (unsigned)P && (fl[p] & 1);
            const unsigned long long m = __ballot(keep);
            const int at = n + ev2g_lanes_below(m);
            if (keep && at < P) nq[at] = p;
            n = min(n + __popcll(m), P);   // (the queue never holds more than P distinct ports; the bound only guards the stage)
        }
        ev2g_wave_sync();
        // heuristics.py:58-81: w EVs' worth of power; the front min(int(ceil(w)), len) entries charge, with Python's slice semantics below 0
        const double w = s.setpoint[(long long)ev2g_scn(e, a.scn_off, s.M) * s.T + t] * 1000.0 / a.avg_power;
        const double cw = ceil(w);
        int k;
        if (!(cw < (double)n)) k = n;
        else if (cw >= 0.0) k = (int)cw;
        else k = (cw <= -(double)n) ? 0 : n + (int)cw;
        for (int i = lane; i < k; i += 64) fl[nq[i]] |= 4;
        ev2g_wave_sync();
        // heuristics.py:84-90: 1 / ports_per_charger each, the last of them the fractional remainder when w < k
        const int last = (k > 0 && w < (double)k) ? nq[k - 1] : -1;
        const double full = 1.0 / (double)s.npc, rest = w - (double)(k - 1);
        double *act = actions + (long long)e * P;
        for (int p = lane; p < P; p += 64) act[p] = (fl[p] & 4) ? (p == last ? rest : full) : 0.0;
        // the k entries that charged move to the back of the queue
        for (int i = lane; i < n; i += 64) {
            const int j = i + k;
            q[i] = nq[j < n ? j : j - n];
        }
        if (lane == 0) a.qlen[e] = n;
    }
}
