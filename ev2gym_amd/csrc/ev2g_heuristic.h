// ev2g_heuristic.h -- the reference's env-reading heuristic agents (ev2gym/baselines/heuristics.py) evaluated on the device state.
//
// One launch computes the actions [E, P] (reference port order) the agent would choose for the current step t, from the engine's
// persistent state as it stands before step t: every port's PortLine and the scenario arrays of DevScn.  Nothing is read from the
// host (after ev2g_pool_refill the host holds no copy of the scenarios).
//   kind 0  ChargeAsLateAsPossible                   heuristics.py:98-149   one lane per (env, port)
//   kind 1  ChargeAsFastAsPossibleToDesiredCapacity  heuristics.py:230-267  one lane per (env, port)
//   kind 2  RoundRobin                               heuristics.py:7-96     one wavefront per env: the agent's queue of port ids lives in
//           HeurArgs::queue between calls and is staged in LDS; every order-preserving pass is an in-order compaction (ballot + prefix count)
//   kind 3  ChargeAsLateAsPossibleToDesiredCapacity  heuristics.py:561-622  one lane per (env, port)
//   kind 4  RoundRobin_GF                            heuristics.py:270-399  one wavefront per env, RoundRobin's queue passes; every queue
//   kind 5  RoundRobin_GF_off_allowed                heuristics.py:402-530  entry carries the min_power / max_power it was INSERTED with
//           (HeurArgs::qmin / qmax, moved with the port ids): the reference computes them from the EV parked at that moment and keeps them
//           while the port stays queued, so a port whose next EV arrives the step after the last one left keeps the old EV's powers.  The
//           selection is the reference's sequential float64 accumulation in queue order (a tree sum rounds differently and flips its `>`):
//           the wavefront reads 64 entries at a time and every lane adds them one by one, lane 0's first (the plain left-to-right sum
//           Python's sum() is before CPython 3.12; later interpreters compensate float sums).  The reference indexes its
//           per-CHARGER max_cs_power with a PORT id, so these two kinds exist for one-port chargers only (ev2g_heuristic_create refuses others).
// A port holds an EV when its window covers t and its session list is not exhausted (ev2g_peek's port_session); that EV's
// current_capacity is the line's `cap`.  Every expression keeps the reference's operation order (-ffp-contract=off): a one-ulp
// difference flips a ceil or a `<` and with it an action.
#pragma once
#include "ev2g_device.h"

#define EV2G_HEUR_BLOCK 256
#define EV2G_HEUR_CALP 0
#define EV2G_HEUR_CAFTDC 1
#define EV2G_HEUR_RR 2
#define EV2G_HEUR_CALPDC 3
#define EV2G_HEUR_RRGF 4
#define EV2G_HEUR_RRGF_OFF 5

struct HeurArgs {
    const int *port_slot;   // [P] slot of every reference port
    const double *cs_kw;    // [C] max_charge_current * voltage * sqrt(phases) / 1000, in that order (EV_Charger.get_max_power)
    double avg_power;       // RoundRobin.average_power: sequential sum over chargers of I * V * sqrt(phases) / n_ports, divided by C
    int *queue;             // [E, P] RoundRobin's ev_buffer of every env (port ids, next to be served first)
    int *qlen;              // [E]
    int scn_off;            // env e runs scenario (e + scn_off) mod M
    const double *cs_min_kw;   // [C] min_charge_current * voltage * sqrt(phases) / 1000 (EV_Charger.get_min_charge_power)
    double min_action;         // RoundRobin_GF.min_action: the LAST charger's min_charge_current / max_charge_current + 1e-4
    double *qmin, *qmax;       // [E, P] RoundRobin_GF*'s min_power / max_power lists, entry for entry next to `queue`
};

// LDS bytes of one env's RoundRobin stage: the new queue (int [P]) and a flag byte per port, 16-byte aligned
__host__ __device__ inline size_t ev2g_heur_rr_wave_bytes(int P) { return ((size_t)P * 4 + (size_t)P + 15) & ~(size_t)15; }
// ... and of one env's RoundRobin_GF* stage: the new min_power and max_power lists (double [P] each) in front of those two
__host__ __device__ inline size_t ev2g_heur_gf_wave_bytes(int P) { return (size_t)P * 16 + ev2g_heur_rr_wave_bytes(P); }

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

// lane j's value of `v` (j is the same in every lane)
__device__ __forceinline__ double ev2g_lane_value(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
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
    constexpr bool GF = KIND == EV2G_HEUR_RRGF || KIND == EV2G_HEUR_RRGF_OFF;
    if constexpr (KIND != EV2G_HEUR_RR && !GF) {
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
            } else if constexpr (KIND == EV2G_HEUR_CALPDC) {   // heuristics.py:583-604
                const double B = s.ss_B[ss];
                const double desired_soc = s.ss_des[ss] / B, soc = cap / B;
                const double x = (desired_soc - soc) / (pw * ts / 60.0 / B);   // steps at full power, the last one fractional
                if (soc < desired_soc && (double)t_dep - ceil(x) <= (double)t) v = (x < 1.0) ? x : 1.0;
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
        unsigned char *stage = heur_lds + (size_t)wave * (GF ? ev2g_heur_gf_wave_bytes(P) : ev2g_heur_rr_wave_bytes(P));
        double *nmin = (double *)stage, *nmax = nmin + P;   // RoundRobin_GF*: the new queue's min_power / max_power
        int *nq = GF ? (int *)(nmax + P) : (int *)stage;    // the new queue
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
            if (add) {
                const int at = n + __popcll((m >> lane) >> 1);   // the lanes above this one come first
                nq[at] = p;
                if constexpr (GF) {   // heuristics.py:311-314: the powers of the EV that is parked now stay with the entry
                    int slot, t_dep;
                    double cap;
                    const int ss = ev2g_heur_port(s, st, a, e, p, t, slot, cap, t_dep);
                    const int cs = s.slot_cs[slot];
                    const double cs_lo = a.cs_min_kw[cs], ev_lo = s.ss_pacmin[ss], cs_hi = a.cs_kw[cs], ev_hi = s.ss_pacmax[ss];
                    nmin[at] = (ev_lo > cs_lo) ? ev_lo : cs_lo;   // max(charger, EV): the first argument unless the second is larger
                    nmax[at] = (ev_hi < cs_hi) ? ev_hi : cs_hi;   // min(charger, EV)
                }
            }
            n += __popcll(m);
        }
        // ... followed by the queued ports that still want charge, in their order (the others are removed)
        for (int base = 0; base < len; base += 64) {
            const int i = base + lane;
            const int p = (i < len) ? q[i] : -1;
            const bool keep = (unsigned)p < (unsigned)P && (fl[p] & 1);
            const unsigned long long m = __ballot(keep);
            const int at = n + ev2g_lanes_below(m);
            if (keep && at < P) {
                nq[at] = p;
                if constexpr (GF) {
                    nmin[at] = a.qmin[(long long)e * P + i];
                    nmax[at] = a.qmax[(long long)e * P + i];
                }
            }
            n = min(n + __popcll(m), P);   // (the queue never holds more than P distinct ports; the bound only guards the stage)
        }
        ev2g_wave_sync();
        double *act = actions + (long long)e * P;
        int k;
        if constexpr (!GF) {
            // heuristics.py:58-81: w EVs' worth of power; the front min(int(ceil(w)), len) entries charge, with Python's slice semantics below 0
            const double w = s.setpoint[(long long)ev2g_scn(e, a.scn_off, s.M) * s.T + t] * 1000.0 / a.avg_power;
            const double cw = ceil(w);
            if (!(cw < (double)n)) k = n;
            else if (cw >= 0.0) k = (int)cw;
            else k = (cw <= -(double)n) ? 0 : n + (int)cw;
            for (int i = lane; i < k; i += 64) fl[nq[i]] |= 4;
            ev2g_wave_sync();
            // heuristics.py:84-90: 1 / ports_per_charger each, the last of them the fractional remainder when w < k
            const int last = (k > 0 && w < (double)k) ? nq[k - 1] : -1;
            const double full = 1.0 / (double)s.npc, rest = w - (double)(k - 1);
            for (int p = lane; p < P; p += 64) act[p] = (fl[p] & 4) ? (p == last ? rest : full) : 0.0;
        } else {
            // heuristics.py:352-364 / 484-495: entries are taken from the front until the running total exceeds the setpoint (kW).  The total
            // is accumulated entry by entry in queue order, in every lane alike: GF starts from sum(min_power) and adds max - min per entry,
            // the off-allowed variant starts from 0 and adds max
            const double sp = s.setpoint[(long long)ev2g_scn(e, a.scn_off, s.M) * s.T + t];
            double total = 0.0;
            if constexpr (KIND == EV2G_HEUR_RRGF) {
                for (int base = 0; base < n; base += 64) {
                    const double v = (base + lane < n) ? nmin[base + lane] : 0.0;
                    const int cnt = min(64, n - base);
                    for (int j = 0; j < cnt; j++) total += ev2g_lane_value(v, j);
                }
            }
            k = 0;
            bool more = true;
            for (int base = 0; base < n && more; base += 64) {
                const int i = base + lane;
                double v = 0.0;
                if (i < n) v = (KIND == EV2G_HEUR_RRGF) ? nmax[i] - nmin[i] : nmax[i];
                const int cnt = min(64, n - base);
                for (int j = 0; j < cnt; j++) {
                    if (total > sp) { more = false; break; }
                    total += ev2g_lane_value(v, j);
                    k += 1;
                }
            }
            for (int i = lane; i < k; i += 64) fl[nq[i]] |= 4;
            ev2g_wave_sync();
            // heuristics.py:384-394 / 515-525: the chosen ports at 1, the last of them trimmed by the overshoot over ITS max_cs_power entry
            // (indexed by the port id: one port per charger); the others at min_action (GF) or off
            const bool trim = (KIND == EV2G_HEUR_RRGF) ? total >= sp : total > sp;
            const int last = (k > 0 && trim) ? nq[k - 1] : -1;
            const double rest = (last >= 0) ? 1.0 - (total - sp) / a.cs_kw[last] : 0.0;
            const double idle = (KIND == EV2G_HEUR_RRGF) ? a.min_action : 0.0;
            for (int p = lane; p < P; p += 64) act[p] = (fl[p] & 4) ? (p == last ? rest : 1.0) : idle;
        }
        // the k entries that charged move to the back of the queue
        for (int i = lane; i < n; i += 64) {
            const int j = i + k, from = j < n ? j : j - n;
            q[i] = nq[from];
            if constexpr (GF) {
                a.qmin[(long long)e * P + i] = nmin[from];
                a.qmax[(long long)e * P + i] = nmax[from];
            }
        }
        if (lane == 0) a.qlen[e] = n;
    }
}
