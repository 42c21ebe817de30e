// ev2g_records.h -- the plain session records the loader builds on the host and the kernels read on the device.  No HIP header: the same
// definitions compile with a plain C++17 host compiler (ev2g_load_host.h, tests/host/load_plan_check.cpp) and inside the device code
// (ev2g_device.h includes this file).
#pragma once
#include <stdint.h>

#ifndef EV2G_HD
#if defined(__HIPCC__)
#define EV2G_HD __host__ __device__ inline
#else
#define EV2G_HD inline
#endif
#endif

#define EV2G_INT_MAX 0x7fffffff

// One EV session, 128 bytes = one cache line: what the per-step battery maths and an arrival need (ev.py:68-113), laid out by CONSUMER so that
// each of them fetches a contiguous run of 16-byte chunks: a charging step reads chunks 0..4 (80 bytes), a discharging step chunks 3..6
// (64 bytes), an arrival chunks 2 and 7.  `rB` / `rv` are the correctly rounded reciprocals of `B` / `v` (computed once per session, by the
// loader or the device generator, with an IEEE division): the battery maths divides by B and v through them (ev2g_fdiv2, ev2g_device.h)
// instead of through ~11-instruction hardware division sequences.
struct __attribute__((aligned(128))) SessRec {
    double pacmax, ts;        // chunk 0  (charge)
    double tsm, eta_ch;       // chunk 1  (charge)
    double gate_ch;           // chunk 2  (charge)  min_ac_charge_power*1000/(voltage*sqrt(charger phases))   (ev.py:151)
    double B;                 //          (charge, arrival)
    double rB;                // chunk 3  (charge)  RN(1 / B)
    double v;                 //          (charge, discharge)  voltage*sqrt(min(charger phases, ev_phases))   (ev.py:169,279,365)
    double rv;                // chunk 4  (charge, discharge)  RN(1 / v)
    double gate_dis;          //          (discharge)  min_discharge_power*1000/(voltage*sqrt(charger phases))   (ev.py:153)
    double minB, emerg;       // chunk 5  (discharge)
    double pdismax, eta_dis;  // chunk 6  (discharge)
    double cap0;              // chunk 7  (arrival)  battery_capacity_at_arrival
    double potc;              //          (arrival)  this EV's term of calculate_charge_power_potential before the charger clamp:
                              //          v * min(pacmax*1000/v, charger max current) / 1000   (utils.py:773-777), evaluated once per session
};
static_assert(sizeof(SessRec) == 128 && alignof(SessRec) == 128, "SessRec is one 128-byte cache line (DESIGN.md, section 2)");
// What a departure reads (and the rewards that look at every connected EV's desired capacity), 16 bytes per session next to the records
struct SessTail {
    double des;          // desired_capacity
    int nt_arr, nt_dep;  // window of the next session on the same port (EV2G_INT_MAX = none)
};
static_assert(sizeof(SessTail) == 16, "SessTail is 16 bytes");

// Round 5: the battery maths' operands that are the SAME for every session of one car model on one kind of charger (ev.py:68-113: the model's
// powers, battery size, gates; the charger's voltage and phases) live in a small dictionary instead of in every session's record: a few
// dozen 128-byte entries that stay in the vector L1, so the fetch in the middle of the battery-maths phase is an L1 hit instead of an L2
// round trip to the session's own line (the one lever that reached 0.60 of the roofline in round 4's ablation).  What really differs per
// session -- transition_soc and, without an efficiency table, the two efficiencies (utils.py:293-296,309-310) -- is SessDyn: it travels with the
// arrival's other operands into the port's LDS state (ev2g_step_wave.h) and, across launches, into the port's PortDyn entry.
// Laid out by consumer: a charging step reads chunks 0..3 (one 64-byte sector), a discharging step chunks 4..6.
struct __attribute__((aligned(128))) ClsRec {
    double pacmax, tsm;       // chunk 0  (charge)
    double gate_ch, B;        // chunk 1  (charge)
    double rB, v;             // chunk 2  (charge)
    double rv, pad0;          // chunk 3  (charge)
    double v_d, rv_d;         // chunk 4  (discharge: copies of v, rv)
    double gate_dis, minB;    // chunk 5  (discharge)
    double emerg, pdismax;    // chunk 6  (discharge)
    double pad1[2];
};
static_assert(sizeof(ClsRec) == 128 && alignof(ClsRec) == 128 && __builtin_offsetof(ClsRec, v_d) == 64,
              "ClsRec is two 64-byte halves: charge operands, discharge operands (DESIGN.md, section 2)");
#define EV2G_CLS_CAP 4096     // dictionary entries (12 bits of the port's LDS word); a batch with more distinct tuples keeps one ClsRec per SESSION instead
struct __attribute__((aligned(32))) SessDyn {
    double ts, eta_ch;        // EV.transition_soc, EV.charge_efficiency (a number: sessions without an efficiency table)
    double eta_dis;           // EV.discharge_efficiency
    int lut, cls;             // efficiency-table id (-1: none), dictionary entry (the session's own index when the batch has no dictionary)
};
static_assert(sizeof(SessDyn) == 32, "SessDyn is four words");
EV2G_HD ClsRec ev2g_cls_of(const SessRec &r) {
    ClsRec c;
    c.pacmax = r.pacmax; c.tsm = r.tsm; c.gate_ch = r.gate_ch; c.B = r.B; c.rB = r.rB; c.v = r.v; c.rv = r.rv; c.pad0 = 0.0;
    c.v_d = r.v; c.rv_d = r.rv; c.gate_dis = r.gate_dis; c.minB = r.minB; c.emerg = r.emerg; c.pdismax = r.pdismax; c.pad1[0] = 0.0; c.pad1[1] = 0.0;
    return c;
}
