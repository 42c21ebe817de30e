// ev2g_load_host.h -- the host-only half of ev2g_load_scenarios: everything the loader computes before it touches the device.
//
// A reference-shaped batch (chargers, transformers, EVs_profiles-ordered sessions) becomes a LoadPlan: transformer-major port slots,
// sessions in (scenario, slot, arrival) order with the next session's window chained in, per-port first-session tables, the charger
// constants, the session records and the battery-maths dictionary.  ev2g_host.hip routes the plan to a kernel, uploads it and allocates
// the state (its load_* functions).  Nothing here needs HIP, a handle or a kernel header, so a plain C++17 program can build plans and
// check them (tests/host/load_plan_check.cpp).  Compile with -ffp-contract=off, like the library: the constants follow the reference's
// operation order.
//
// Every load_plan_* function that can refuse a batch returns EV2G_OK or an EV2G_ERR_* code with the message in `msg`; they run in the
// order they are declared in, each reading what the earlier ones left in the plan.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ev2g.h"
#include "ev2g_records.h"

// The loader's environment switches (A/B runs, routing and parity tests), read once per load.
struct LoadSwitches {
    long long pool_session_cap = 0;   // EV2G_POOL_SESSION_CAP: at least this many session slots per scenario of a refillable pool
    bool no_full = false, no_wide = false, no_strided = false;   // EV2G_NO_FULL / EV2G_NO_WIDE / EV2G_NO_STRIDED
    bool no_inl_stats = false;        // EV2G_NO_INLAUNCH_STATS
    bool no_fast_forward = false;     // EV2G_NO_FAST_FORWARD: every EV-free step of a persistent launch is stepped
    bool no_cu_balance = false;       // EV2G_NO_CU_BALANCE: every launch keeps the kernel's own workgroup -> env group map
    bool placement = false;          // EV2G_PLACEMENT: fast-forwarding launches record where their workgroups ran (ev2g_last_launch_placement)
    bool kernel_v2 = false;           // EV2G_KERNEL=v2: the general kernel on the common shape
    bool no_dict = false;             // EV2G_NO_DICT: one ClsRec per session
    bool no_big = false;              // EV2G_NO_BIG: ev2g_step_v2<1024> where ev2g_step_big would run
    bool timing_events = false;       // EV2G_LAUNCH_TIMING=events: every timed call keeps its HIP-event pair (ev2g_timing_host.h), no launch stamps
};
inline LoadSwitches load_switches_from_env() {
    LoadSwitches sw;
    if (const char *e = std::getenv("EV2G_POOL_SESSION_CAP")) sw.pool_session_cap = std::atoll(e);
    sw.no_full = std::getenv("EV2G_NO_FULL") != nullptr;
    sw.no_wide = std::getenv("EV2G_NO_WIDE") != nullptr;
    sw.no_strided = std::getenv("EV2G_NO_STRIDED") != nullptr;
    sw.no_inl_stats = std::getenv("EV2G_NO_INLAUNCH_STATS") != nullptr;
    sw.no_fast_forward = std::getenv("EV2G_NO_FAST_FORWARD") != nullptr;
    sw.no_cu_balance = std::getenv("EV2G_NO_CU_BALANCE") != nullptr;
    sw.placement = std::getenv("EV2G_PLACEMENT") != nullptr;
    const char *kn = std::getenv("EV2G_KERNEL");
    sw.kernel_v2 = kn && std::string(kn) == "v2";
    sw.no_dict = std::getenv("EV2G_NO_DICT") != nullptr;
    sw.no_big = std::getenv("EV2G_NO_BIG") != nullptr;
    const char *lt = std::getenv("EV2G_LAUNCH_TIMING");
    sw.timing_events = lt && std::string(lt) == "events";
    return sw;
}

// The battery-maths dictionary's host side: a ClsRec's eleven operands, bit for bit -> its entry
typedef std::array<uint64_t, 11> ClsKey;
// dictionary entry of a ClsRec (by value, bit for bit); -1 when the dictionary is full
inline int cls_find_or_add(std::map<ClsKey, int> &map, std::vector<ClsRec> &tab, const ClsRec &c) {
    ClsKey k;
    const double f[11] = {c.pacmax, c.tsm, c.gate_ch, c.B, c.rB, c.v, c.rv, c.gate_dis, c.minB, c.emerg, c.pdismax};
    std::memcpy(k.data(), f, sizeof f);
    auto it = map.find(k);
    if (it != map.end()) return it->second;
    if (map.size() >= EV2G_CLS_CAP) return -1;
    const int id = (int)map.size();
    map.emplace(k, id);
    if ((size_t)id >= tab.size()) tab.resize((size_t)id + 1);
    tab[(size_t)id] = c;
    return id;
}

// The constants of a session's record that depend on its charger, from r.B and r.pacmax and the charger's row `vk` of cs_vk
// (voltage * sqrt(k), k = 0..3).  The loader and ev2g_pool_refill's dictionary entries both come from here (and ev2g_refill.h's
// write_session forms the same on the device): a refilled pool is bit-identical to a loaded one only while they agree.
inline void ev2g_sess_consts(SessRec &r, const double *vk, int cs_phases, int ev_phases, double pac_min, double pdis_min, double cs_imax) {
    const double v_gate = vk[cs_phases];
    r.gate_ch = pac_min * 1000.0 / v_gate;
    r.gate_dis = pdis_min * 1000.0 / v_gate;
    r.v = vk[std::min(cs_phases, ev_phases)];
    r.rB = 1.0 / r.B; r.rv = 1.0 / r.v;   // correctly rounded reciprocals (IEEE division): what ev2g_fdiv2 divides through
    // this EV's charge-power-potential term before the charger clamp (utils.py:773-777), the reference's operations in its order
    const double evc = r.pacmax * 1000.0 / r.v;
    r.potc = r.v * ((evc < cs_imax) ? evc : cs_imax) / 1000.0;
}

struct IntPair { int x, y; };   // (uploaded as int2)

struct LoadPlan {
    // ---- sizes (load_plan_check; D, cap, SD: load_plan_layout) ----
    int E = 0, M = 0, T = 0, C = 0, npc = 0, P = 0, R = 0, D = 0, ND = 0;   // E envs stepped concurrently, M scenarios in the pool
    int dt = 0, n_lut = 0;              // minutes per step, efficiency tables
    long long S = 0, SD = 0, cap = 0;   // sessions of the batch; device session slots (holes of a refillable pool included); slots per scenario (0: packed)
    bool het = false;                   // chargers with different port counts (topology file)
    // ---- layout ----
    std::vector<int> np_of, pbase;      // [C] ports of each charger, [C+1] its first port (numbered like the reference's port_counter)
    std::vector<int> slot_port, slot_cs, slot_tr, slot_obs, slot_mask, port_slot, cs_slot0, tr_seg, tr_obs;
    int max_seg = 1;
    std::vector<int> scn_sess, scn_sess_end;   // device sessions of scenario m: [scn_sess[m], scn_sess_end[m]) (device order is scenario-major)
    // ---- session order ----
    std::vector<int> sess_port, host_to_dev;   // [S] host order: resolved reference port, device session index
    std::vector<long long> dev_to_host;        // [SD] -1: an unused slot of a refillable pool
    std::vector<int> ss_slot;                  // [SD] port slot of a session
    std::vector<int> port_first, port_end;     // [M*P] a port's sessions are consecutive in device order: first, one past the last (-1: none)
    std::vector<IntPair> port_first_win;       // [M*P] window of the port's first session (EV2G_INT_MAX: none)
    // ---- session fields in device order, constants, records ----
    std::vector<int> ss_tarr, ss_tdep, ss_ntarr, ss_ntdep, ss_phases, ss_lut;
    std::vector<double> ss_cap0, ss_B, ss_des, ss_minB, ss_emerg, ss_pacmax, ss_pacmin, ss_pdismax, ss_pdismin, ss_ts, ss_tsm, ss_etach, ss_etadis;
    std::vector<double> cs_maxp, cs_minp, cs_vk, cs_dmax_abs, cs_pack;
    std::vector<double> cs_kw, cs_min_kw;      // the heuristic agents' charger constants, in the reference's operation order
    double avg_power = 0.0, min_action = 0.0;
    std::vector<double> tr_peak, tr_base, lut_eta, rowmax;
    std::vector<double> ss_afap, sess_afap_host;   // max_energy_AFAP: device order [SD], host order [S]
    std::vector<SessRec> recs;
    std::vector<SessTail> tails;
    // ---- dictionary (fast path) ----
    std::vector<SessDyn> dyns;
    std::vector<ClsRec> cls_tab;
    std::map<ClsKey, int> cls_map;
    bool dict = false;
    // ---- ev2g_step_big's charger classes, potential table and eligibility facts ----
    std::vector<unsigned char> ccls;
    std::vector<double> ctab, ptab;
    bool many = false, even = false;
    int tmax = 0, tmin = 0;
};

// The shape checks that leave a loaded pool untouched when they refuse; fills the sizes, np_of and pbase.
inline int load_plan_check(LoadPlan &p, const ev2g_scenario_batch *b, const ev2g_config &cfg, std::string &msg) {
    const int M = b->n_envs, T = b->n_steps, C = b->n_chargers, npc = b->ports_per_charger, R = b->n_transformers;
    auto refuse = [&](const char *m) { msg = m; return EV2G_ERR_ARG; };
    p.M = M; p.T = T; p.C = C; p.npc = npc; p.R = R; p.dt = b->timescale; p.n_lut = b->n_lut;
    p.ND = std::max(b->n_dr_max, 0);
    p.E = cfg.n_active_envs > 0 ? cfg.n_active_envs : M;
    if (p.E > M) return refuse("ev2g_load_scenarios: n_active_envs exceeds the number of scenarios in the batch");
    if (M <= 0 || T <= 0 || C <= 0 || npc <= 0 || R <= 0 || b->timescale <= 0) return refuse("ev2g_load_scenarios: non-positive size");
    if (b->horizon != 20) return refuse("ev2g_load_scenarios: horizon must be 20 (state.py:119,129-132)");
    if (npc > 32) return refuse("ev2g_load_scenarios: more than 32 ports per charger unsupported");
    // ports of each charger: uniform, or per charger from a topology file (loaders.py:312-340); numbered cumulatively in charger
    // order like the reference's port_counter (ev2gym_env.py:364-385)
    p.np_of.assign(C, npc); p.pbase.assign(C + 1, 0);
    p.het = false;
    if (b->cs_n_ports) {
        int mx = 0;
        for (int c = 0; c < C; c++) {
            p.np_of[c] = b->cs_n_ports[c];
            if (p.np_of[c] < 1) return refuse("ev2g_load_scenarios: cs_n_ports must be >= 1");
            mx = std::max(mx, p.np_of[c]);
            p.het = p.het || p.np_of[c] != npc;
        }
        if (mx != npc) return refuse("ev2g_load_scenarios: ports_per_charger must be the maximum of cs_n_ports");
    }
    for (int c = 0; c < C; c++) p.pbase[c + 1] = p.pbase[c] + p.np_of[c];
    const int P = p.P = p.pbase[C];
    if (p.het)   // the reference's action mask is indexed i*cs.n_ports + j (ev2gym_env.py:452-457): past the array it raises IndexError
        for (int c = 0; c < C; c++)
            if (c * p.np_of[c] + p.np_of[c] > P)
                return refuse("ev2g_load_scenarios: this charger order makes the reference's action mask index "
                              "i*n_ports+j leave the mask array (ev2gym_env.py:457 raises IndexError); order the chargers by falling port count");
    const long long S = p.S = b->env_session_start[M];
    if (S != b->n_sessions || b->env_session_start[0] != 0) return refuse("ev2g_load_scenarios: env_session_start inconsistent with n_sessions");
    if (S > 0x7ffffff0LL) return refuse("ev2g_load_scenarios: too many sessions for 32-bit indices");
    {   // the kernels index with 32-bit ints: every element offset they form must stay below 2^31
        const long long lim = 0x7fffffffLL, Pq = P;
        const long long Dq = 3 + 3 * Pq > 22 + 40LL * R + 2 * Pq ? 3 + 3 * Pq : 22 + 40LL * R + 2 * Pq;
        const bool log_cs = (cfg.flags & EV2G_FLAG_LOG_CS_HISTORY) != 0;
        if ((long long)M * Pq > lim || (long long)M * Dq > lim || (long long)M * R * (T + 1) * 40 > lim ||
            (log_cs && (long long)T * M * std::max<long long>(C, Pq) > lim) || (long long)M * T * 8 > lim)
            return refuse("ev2g_load_scenarios: batch too large for 32-bit element offsets "
                          "(need M*P, M*D, M*R*(T+1)*40, T*M*C < 2^31): split it over more handles / GPUs");
    }
    if (T > 65535 || b->n_lut > 65534)
        return refuse("ev2g_load_scenarios: simulation_length and the number of efficiency tables must stay below 65536 (a port's state line "
                      "packs charging_cycles and the table id into 16 bits each)");
    for (int c = 0; c < C; c++) {
        if (b->cs_transformer[c] < 0 || b->cs_transformer[c] >= R) return refuse("ev2g_load_scenarios: cs_transformer out of range");
        if (b->cs_phases[c] < 1 || b->cs_phases[c] > 3) return refuse("ev2g_load_scenarios: cs_phases must be 1..3");
    }
    return EV2G_OK;
}

// Slot order (transformer-major, chargers in id order inside a transformer, ports adjacent), the observation columns of the state
// function, and the device session storage.  Packed (default): scenario m owns the device sessions [env_session_start[m],
// env_session_start[m+1]).  EV2G_FLAG_REFILLABLE: every scenario owns a fixed-size block of `cap` session slots (the largest count of the
// batch + 25 % + 8, or EV2G_POOL_SESSION_CAP), so that ev2g_pool_refill can regenerate a scenario in place on the device; SD counts slots,
// holes included.
inline int load_plan_layout(LoadPlan &p, const ev2g_scenario_batch *b, const ev2g_config &cfg, const LoadSwitches &sw, std::string &msg) {
    const int M = p.M, C = p.C, P = p.P, R = p.R;
    for (auto *v : {&p.slot_port, &p.slot_cs, &p.slot_tr, &p.slot_obs, &p.slot_mask, &p.port_slot}) v->assign(P, 0);
    p.tr_seg.assign(R + 1, 0); p.tr_obs.assign(R, 0);
    int q = 0;
    for (int r = 0; r < R; r++) {
        p.tr_seg[r] = q;
        for (int c = 0; c < C; c++)
            if (b->cs_transformer[c] == r)
                for (int j = 0; j < p.np_of[c]; j++) {
                    p.slot_port[q] = p.pbase[c] + j;
                    p.slot_mask[q] = c * p.np_of[c] + j;   // where the reference sets this port's action-mask entry (ev2gym_env.py:457)
                    p.slot_cs[q] = c;
                    p.slot_tr[q] = r;
                    p.port_slot[p.pbase[c] + j] = q;
                    q++;
                }
    }
    p.tr_seg[R] = q;
    p.cs_slot0.resize(C);
    for (int c = 0; c < C; c++) p.cs_slot0[c] = p.port_slot[p.pbase[c]];
    if (cfg.state_kind == EV2G_STATE_PUBLIC_PST) {
        p.D = 3 + 3 * P;
        for (q = 0; q < P; q++) p.slot_obs[q] = 3 + 3 * q;
    } else if (cfg.state_kind == EV2G_STATE_V2G_PROFIT_MAX) {
        p.D = 22 + 2 * P;
        for (q = 0; q < P; q++) p.slot_obs[q] = 22 + 2 * q;
    } else {
        p.D = 22 + 40 * R + 2 * P;
        for (int r = 0; r < R; r++) p.tr_obs[r] = 22 + 40 * r + 2 * p.tr_seg[r];
        for (q = 0; q < P; q++) p.slot_obs[q] = 22 + 40 * (p.slot_tr[q] + 1) + 2 * q;
    }
    p.max_seg = 1;
    for (int r = 0; r < R; r++) p.max_seg = std::max(p.max_seg, p.tr_seg[r + 1] - p.tr_seg[r]);

    const bool refillable = (cfg.flags & EV2G_FLAG_REFILLABLE) != 0;
    long long cap = 0;
    if (refillable) {
        for (int m = 0; m < M; m++) cap = std::max<long long>(cap, b->env_session_start[m + 1] - b->env_session_start[m]);
        cap = ((cap + cap / 4 + 8) + 7) / 8 * 8;
        cap = std::max(cap, sw.pool_session_cap);
        if (cap * M > 0x7ffffff0LL) { msg = "ev2g_load_scenarios: too many session slots for 32-bit indices (refillable pool)"; return EV2G_ERR_ARG; }
    }
    p.cap = cap;
    p.SD = refillable ? cap * M : p.S;
    p.scn_sess.resize((size_t)M + 1); p.scn_sess_end.resize((size_t)M);
    for (int m = 0; m <= M; m++) p.scn_sess[(size_t)m] = refillable ? (int)(cap * m) : (int)b->env_session_start[m];
    for (int m = 0; m < M; m++) p.scn_sess_end[(size_t)m] = p.scn_sess[(size_t)m] + (int)(b->env_session_start[m + 1] - b->env_session_start[m]);
    return EV2G_OK;
}

// Resolves every session's port (the reference's first-free replay, ev_charger.py:266-286) and orders the sessions by (scenario, slot, arrival).
inline int load_plan_order(LoadPlan &p, const ev2g_scenario_batch *b, std::string &msg) {
    const int M = p.M, C = p.C, npc = p.npc, P = p.P;
    auto refuse = [&](const char *m) { msg = m; return EV2G_ERR_ARG; };
    p.sess_port.assign((size_t)p.S, 0); p.host_to_dev.assign((size_t)p.S, 0);
    p.ss_slot.assign((size_t)std::max<long long>(p.SD, 1), 0);
    p.dev_to_host.assign((size_t)p.SD, -1);
    p.port_first.assign((size_t)M * P, -1);
    p.port_end.assign((size_t)M * P, -1);
    p.port_first_win.assign((size_t)M * P, IntPair{EV2G_INT_MAX, EV2G_INT_MAX});
    std::vector<int> free_at((size_t)C * npc);
    std::vector<std::pair<long long, long long>> keyed;  // (slot, host idx)
    for (int e = 0; e < M; e++) {
        long long d = p.scn_sess[(size_t)e];
        std::fill(free_at.begin(), free_at.end(), 0);
        const long long s0 = b->env_session_start[e], s1 = b->env_session_start[e + 1];
        if (s1 < s0) return refuse("ev2g_load_scenarios: env_session_start not monotone");
        keyed.clear();
        int prev_arr = 0;
        for (long long s = s0; s < s1; s++) {
            const int cs = b->ev_cs[s], ta = b->ev_t_arr[s], td = b->ev_t_dep[s];
            if (cs < 0 || cs >= C) return refuse("ev2g_load_scenarios: ev_cs out of range");
            if (ta < 1 || td < ta) return refuse("ev2g_load_scenarios: need 1 <= t_arr <= t_dep");
            if (ta < prev_arr) return refuse("ev2g_load_scenarios: sessions must be sorted by arrival");
            if (b->ev_phases[s] < 1 || b->ev_phases[s] > 3) return refuse("ev2g_load_scenarios: ev_phases must be 1..3");
            if (b->ev_lut[s] >= b->n_lut) return refuse("ev2g_load_scenarios: ev_lut out of range");
            prev_arr = ta;
            int slot = -1;
            for (int j = 0; j < p.np_of[cs]; j++)
                if (free_at[(size_t)cs * npc + j] <= ta - 1) {  // attached at the end of step ta-1
                    slot = j;
                    break;
                }
            if (slot < 0) return refuse("ev2g_load_scenarios: no free port for a session (assert n_evs_connected < n_ports, ev_charger.py:271)");
            free_at[(size_t)cs * npc + slot] = td;  // freed inside step td, before that step's spawns
            p.sess_port[s] = p.pbase[cs] + slot;
            keyed.emplace_back((long long)p.port_slot[p.pbase[cs] + slot], s);
        }
        std::stable_sort(keyed.begin(), keyed.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
        for (auto &kv : keyed) {
            p.host_to_dev[kv.second] = (int)d;
            p.dev_to_host[d] = kv.second;
            p.ss_slot[(size_t)d] = (int)kv.first;
            const size_t g = (size_t)e * P + kv.first;
            if (p.port_first[g] < 0) {
                p.port_first[g] = (int)d;
                p.port_first_win[g] = IntPair{b->ev_t_arr[kv.second], b->ev_t_dep[kv.second]};
            }
            p.port_end[g] = (int)d + 1;
            d++;
        }
    }
    return EV2G_OK;
}

// EV.calculate_max_energy_with_AFAP (ev.py:407-440)
inline double afap_energy(const ev2g_scenario_batch *b, long long s, double max_cs_power) {
    const double pac = b->ev_pac_max[s];
    const double max_power = (std::fabs(max_cs_power) > std::fabs(pac)) ? pac : max_cs_power;
    double eff;
    if (b->ev_lut[s] >= 0) {
        double m = 0;
        for (int k = 0; k < EV2G_LUT_LEN; k++) m = std::max(m, b->lut[(size_t)b->ev_lut[s] * EV2G_LUT_LEN + k]);
        eff = m / 100.0;
    } else
        eff = b->ev_eta_ch[s];
    double x = b->ev_cap0[s];
    for (int k = b->ev_t_arr[s]; k < b->ev_t_dep[s] + 1; k++) {
        x += max_power * eff * b->timescale / 60.0;
        x = std::ceil(x * 100.0) / 100.0;
        if (x > b->ev_B[s]) {
            x = b->ev_B[s];
            break;
        }
    }
    return x;
}

// The charger constants, the per-scenario tables the host derives, and the session records.
inline void load_plan_constants(LoadPlan &p, const ev2g_scenario_batch *b) {
    const int M = p.M, T = p.T, C = p.C, R = p.R;
    p.cs_maxp.resize(C); p.cs_minp.resize(C); p.cs_vk.resize((size_t)C * 4); p.cs_dmax_abs.resize(C);
    for (int c = 0; c < C; c++) {
        const double V = b->cs_voltage[c];
        for (int k = 0; k < 4; k++) p.cs_vk[(size_t)c * 4 + k] = V * std::sqrt((double)k);
        const double sq = std::sqrt((double)b->cs_phases[c]);
        p.cs_maxp[c] = sq * V * b->cs_max_charge_current[c] / 1000;  // utils.py:779-782
        p.cs_minp[c] = sq * V * b->cs_min_charge_current[c] / 1000;
        p.cs_dmax_abs[c] = std::fabs(b->cs_max_discharge_current[c]);
    }
    // the heuristic agents' charger constants, evaluated like the reference: EV_Charger.get_max_power / get_min_charge_power
    // (ev_charger.py:251-255), RoundRobin.average_power (heuristics.py:19-24) and RoundRobin_GF.min_action (heuristics.py:285-286:
    // the loop leaves the LAST charger's) -- not cs_maxp / cs_minp, whose operation order rounds differently
    p.cs_kw.resize(C); p.cs_min_kw.resize(C);
    double total = 0.0;
    for (int c = 0; c < C; c++) {
        const double I = b->cs_max_charge_current[c], V = b->cs_voltage[c], sq = std::sqrt((double)b->cs_phases[c]);
        p.cs_kw[c] = I * V * sq / 1000;
        p.cs_min_kw[c] = b->cs_min_charge_current[c] * V * sq / 1000;
        total += I * V * sq / (double)p.np_of[c];
    }
    p.avg_power = total / (double)C;
    p.min_action = b->cs_min_charge_current[C - 1] / b->cs_max_charge_current[C - 1] + 1e-4;
    // the six per-charger operands of the fast path side by side: (imax, |dmax|), (imin, dmin), (max power, min power)
    p.cs_pack.resize((size_t)C * 6);
    for (int c = 0; c < C; c++) {
        double *r = &p.cs_pack[(size_t)c * 6];
        r[0] = b->cs_max_charge_current[c]; r[1] = p.cs_dmax_abs[c]; r[2] = b->cs_min_charge_current[c];
        r[3] = b->cs_min_discharge_current[c]; r[4] = p.cs_maxp[c]; r[5] = p.cs_minp[c];
    }
    p.tr_peak.resize((size_t)M * R);
    for (size_t er = 0; er < (size_t)M * R; er++) {
        double m = b->tr_max_power[er * T];
        for (int t = 1; t < T; t++) m = std::max(m, b->tr_max_power[er * T + t]);
        p.tr_peak[er] = m;
    }
    p.tr_base.resize((size_t)M * R * T);
    for (size_t i = 0; i < p.tr_base.size(); i++) p.tr_base[i] = b->tr_inflexible_load[i] + b->tr_solar_power[i];
    // the efficiency tables as efficiencies (percent / 100, the division of ev.py:290,379 done once), and the largest entry of every
    // table (percent): what EV.calculate_max_energy_with_AFAP uses (ev.py:418-421); device-side refills need it
    p.lut_eta.resize((size_t)b->n_lut * EV2G_LUT_LEN);
    for (size_t i = 0; i < p.lut_eta.size(); i++) p.lut_eta[i] = b->lut[i] / 100.0;
    p.rowmax.assign((size_t)std::max(b->n_lut, 1), 0.0);
    for (int l = 0; l < b->n_lut; l++)
        for (int k = 0; k < EV2G_LUT_LEN; k++) p.rowmax[l] = std::max(p.rowmax[l], b->lut[(size_t)l * EV2G_LUT_LEN + k]);
}

// The session fields in device order with the next window of the same port chained in, max_energy_AFAP, and the AoS records
// (one cache line each) with their tails.  Needs load_plan_constants' cs_vk.
inline void load_plan_records(LoadPlan &p, const ev2g_scenario_batch *b) {
    const int M = p.M;
    const long long S = p.S, SD = p.SD;
    const std::vector<long long> &dev_to_host = p.dev_to_host;
    auto gather = [&](auto &dst, const auto *src) {
        dst.assign((size_t)SD, 0);
        for (long long d = 0; d < SD; d++) if (dev_to_host[d] >= 0) dst[d] = src[dev_to_host[d]];
    };
    gather(p.ss_tarr, b->ev_t_arr); gather(p.ss_tdep, b->ev_t_dep); gather(p.ss_phases, b->ev_phases); gather(p.ss_lut, b->ev_lut);
    gather(p.ss_cap0, b->ev_cap0); gather(p.ss_B, b->ev_B); gather(p.ss_des, b->ev_desired); gather(p.ss_minB, b->ev_minB);
    gather(p.ss_emerg, b->ev_min_emerg); gather(p.ss_pacmax, b->ev_pac_max); gather(p.ss_pacmin, b->ev_pac_min);
    gather(p.ss_pdismax, b->ev_pdis_max); gather(p.ss_pdismin, b->ev_pdis_min); gather(p.ss_ts, b->ev_ts); gather(p.ss_tsm, b->ev_tsm);
    gather(p.ss_etach, b->ev_eta_ch); gather(p.ss_etadis, b->ev_eta_dis);
    p.ss_ntarr.assign((size_t)SD, EV2G_INT_MAX); p.ss_ntdep.assign((size_t)SD, EV2G_INT_MAX);
    for (long long d = 0; d + 1 < SD; d++) {
        const long long a = dev_to_host[d], c = dev_to_host[d + 1];
        if (a < 0 || c < 0) continue;   // (an unused slot of a refillable pool)
        // same scenario (binary search in env_session_start) and same port => the next device session is this port's next session
        const int64_t *st = b->env_session_start;
        const bool same_env = std::upper_bound(st, st + M + 1, (int64_t)a) == std::upper_bound(st, st + M + 1, (int64_t)c);
        if (same_env && p.sess_port[a] == p.sess_port[c]) {
            p.ss_ntarr[d] = p.ss_tarr[d + 1];
            p.ss_ntdep[d] = p.ss_tdep[d + 1];
        }
    }
    p.ss_afap.assign((size_t)SD, 0.0); p.sess_afap_host.assign((size_t)S, 0.0);
    for (long long s = 0; s < S; s++) {
        const int cs = b->ev_cs[s];
        // EV_Charger.get_max_power (ev_charger.py:251-252)
        const double mp = b->cs_max_charge_current[cs] * b->cs_voltage[cs] * std::sqrt((double)b->cs_phases[cs]) / 1000;
        p.sess_afap_host[s] = afap_energy(b, s, mp);
        p.ss_afap[p.host_to_dev[s]] = p.sess_afap_host[s];
    }
    p.recs.resize((size_t)std::max<long long>(SD, 1));
    p.tails.resize((size_t)std::max<long long>(SD, 1));
    std::memset((void *)p.recs.data(), 0, p.recs.size() * sizeof(SessRec));
    std::memset((void *)p.tails.data(), 0, p.tails.size() * sizeof(SessTail));
    for (long long d = 0; d < SD; d++) {
        const long long hs = dev_to_host[d];
        if (hs < 0) continue;
        const int cs = b->ev_cs[hs];
        SessRec &r = p.recs[d];
        r.B = p.ss_B[d]; r.cap0 = p.ss_cap0[d]; r.minB = p.ss_minB[d]; r.emerg = p.ss_emerg[d];
        r.pacmax = p.ss_pacmax[d]; r.pdismax = p.ss_pdismax[d]; r.ts = p.ss_ts[d]; r.tsm = p.ss_tsm[d];
        r.eta_ch = p.ss_etach[d]; r.eta_dis = p.ss_etadis[d];
        ev2g_sess_consts(r, &p.cs_vk[(size_t)cs * 4], b->cs_phases[cs], p.ss_phases[d], p.ss_pacmin[d], p.ss_pdismin[d], b->cs_max_charge_current[cs]);
        p.tails[d].des = p.ss_des[d]; p.tails[d].nt_arr = p.ss_ntarr[d]; p.tails[d].nt_dep = p.ss_ntdep[d];
    }
}

// Battery-maths dictionary (fast path only: `wave_path` is the router's decision): the distinct (car model x charger kind) operand tuples of
// the batch, numbered by first occurrence in device session order, and per session what is left (SessDyn).  More than EV2G_CLS_CAP tuples
// (arbitrary ev_* arrays through the ABI), or EV2G_NO_DICT: one ClsRec per session, entry = session.
inline void load_plan_dictionary(LoadPlan &p, bool wave_path, const LoadSwitches &sw) {
    const long long SD = p.SD;
    p.dict = wave_path && !sw.no_dict;
    if (!wave_path) return;
    p.dyns.resize((size_t)std::max<long long>(SD, 1));
    std::memset((void *)p.dyns.data(), 0, p.dyns.size() * sizeof(SessDyn));
    for (long long d = 0; d < SD && p.dict; d++) {
        if (p.dev_to_host[d] < 0) continue;
        const int k = cls_find_or_add(p.cls_map, p.cls_tab, ev2g_cls_of(p.recs[d]));
        if (k < 0) { p.dict = false; break; }
        p.dyns[d].cls = k;
    }
    if (!p.dict) {
        p.cls_map.clear();
        p.cls_tab.assign((size_t)std::max<long long>(SD, 1), ClsRec{});
        for (long long d = 0; d < SD; d++) if (p.dev_to_host[d] >= 0) { p.cls_tab[d] = ev2g_cls_of(p.recs[d]); p.dyns[d].cls = (int)d; }
    } else
        p.cls_tab.resize(EV2G_CLS_CAP, ClsRec{});   // room for the classes a device refill may add
    for (long long d = 0; d < SD; d++) {
        if (p.dev_to_host[d] < 0) continue;
        p.dyns[d].ts = p.ss_ts[d]; p.dyns[d].eta_ch = p.ss_etach[d]; p.dyns[d].eta_dis = p.ss_etadis[d]; p.dyns[d].lut = p.ss_lut[d];
    }
}

// ev2g_step_big's inputs (a 512 < P <= 1024 env off the fast path): every slot's charger class among at most `ncc_max` distinct constant
// tuples (`many`: there are more), the first 15 distinct potential terms of the loaded sessions (any other value is fetched from the
// state line), and what the router needs to know about the windows and the observation columns.
inline void load_plan_big(LoadPlan &p, const ev2g_scenario_batch *b, int ncc_max) {
    const int P = p.P;
    p.ccls.assign(P, 0); p.ctab.clear();
    p.many = false;
    for (int q = 0; q < P && !p.many; q++) {
        const int c = p.slot_cs[q];
        const double r[6] = {b->cs_max_charge_current[c], b->cs_min_charge_current[c], b->cs_min_discharge_current[c], p.cs_dmax_abs[c], p.cs_maxp[c], p.cs_minp[c]};
        int k = 0;
        const int n = (int)(p.ctab.size() / 6);
        while (k < n && std::memcmp(&p.ctab[(size_t)k * 6], r, sizeof r) != 0) k++;
        if (k == n) { if (n == ncc_max) { p.many = true; break; } p.ctab.insert(p.ctab.end(), r, r + 6); }
        p.ccls[q] = (unsigned char)k;
    }
    p.tmax = p.T; p.tmin = 0;
    for (long long d = 0; d < p.SD; d++)
        if (p.dev_to_host[d] >= 0) { p.tmax = std::max({p.tmax, p.ss_tarr[d], p.ss_tdep[d]}); p.tmin = std::min({p.tmin, p.ss_tarr[d], p.ss_tdep[d]}); }
    p.even = p.D % 2 == 0;
    for (int q = 0; q < P; q++) p.even = p.even && p.slot_obs[q] % 2 == 0;
    p.ptab.assign(15, std::nan(""));
    int npot = 0;
    for (long long d = 0; d < p.SD && npot < 15; d++) {
        if (p.dev_to_host[d] < 0) continue;
        int k = 0;
        while (k < npot && p.ptab[(size_t)k] != p.recs[d].potc) k++;
        if (k == npot) p.ptab[(size_t)npot++] = p.recs[d].potc;
    }
}
