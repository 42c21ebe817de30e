// load_plan_check.cpp -- builds scenario batches in code, runs the loader's host-only plan (ev2gym_amd/csrc/ev2g_load_host.h) on them and
// checks the plan's index arithmetic against definitions written here independently: the first-free port replay, the (scenario, slot,
// arrival) session order, the next-window chaining, the per-port first-session tables, the class dictionary with its overflow fall-back,
// the holes of a refillable pool, and every refusal with its code and message.  Exits non-zero at the first failure.
//
//   c++ -std=c++17 -O1 -ffp-contract=off tests/host/load_plan_check.cpp -o load_plan_check && ./load_plan_check
//
// (tests/test_load_plan_cpu.py does exactly that; the same source builds with -fsanitize=address,undefined.)
#include <cstdio>

#include "../../ev2gym_amd/csrc/ev2g_load_host.h"

static const char *g_case = "";
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "FAIL [%s] line %d: %s\n", g_case, __LINE__, #cond);            \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

struct Charger { int tr, ports, phases; };
struct Sess { int cs, ta, td, model, phases; };

// a batch that owns its arrays; `model` picks one of a few car models (so that dictionary entries repeat), or a session's own tuple (model < 0)
struct Batch {
    ev2g_scenario_batch b{};
    std::vector<double> imin, imax, dmin, dmax, volt, price, tr_series, tr_dr, lut;
    std::vector<int32_t> phases, trf, nports, tr_ndr, tr_ahead, ev_cs, ev_ta, ev_td, ev_ph, ev_lut;
    std::vector<int64_t> start;
    std::vector<double> cap0, B, des, minB, emerg, pacmax, pacmin, pdismax, pdismin, ts, tsm, etach, etadis;

    Batch(int T, int R, const std::vector<Charger> &cs, const std::vector<std::vector<Sess>> &scn, bool topology = false, int n_lut = 0) {
        const int M = (int)scn.size(), C = (int)cs.size();
        int npc = 0;
        for (const Charger &c : cs) {
            imin.push_back(6.0); imax.push_back(32.0 - 8.0 * (c.phases % 2)); dmin.push_back(-6.0); dmax.push_back(-32.0); volt.push_back(c.phases == 3 ? 400.0 : 230.0);
            phases.push_back(c.phases); trf.push_back(c.tr); nports.push_back(c.ports);
            npc = std::max(npc, c.ports);
        }
        price.assign((size_t)M * T, 0.1);
        tr_series.resize((size_t)M * R * T);
        for (size_t i = 0; i < tr_series.size(); i++) tr_series[i] = 50.0 + (double)(i % 7);
        tr_dr.assign((size_t)M * R * 3, 0.0); tr_ndr.assign((size_t)M * R, 0); tr_ahead.assign((size_t)M * R, 4);
        lut.resize((size_t)n_lut * EV2G_LUT_LEN);
        for (size_t i = 0; i < lut.size(); i++) lut[i] = 80.0 + (double)(i % 15);
        start.push_back(0);
        for (const auto &ss : scn) {
            for (const Sess &s : ss) {
                const long long i = (long long)ev_cs.size();
                const int m = s.model;
                ev_cs.push_back(s.cs); ev_ta.push_back(s.ta); ev_td.push_back(s.td); ev_ph.push_back(s.phases);
                ev_lut.push_back(n_lut > 0 && m >= 0 ? m % n_lut : -1);
                const double Bv = m >= 0 ? 40.0 + 20.0 * (m % 3) : 30.0 + 0.01 * (double)i;
                B.push_back(Bv); cap0.push_back(0.3 * Bv + 0.001 * (double)(i % 11)); des.push_back(0.9 * Bv); minB.push_back(0.1 * Bv); emerg.push_back(0.15 * Bv);
                pacmax.push_back(m >= 0 ? 7.4 + 3.6 * (m % 3) : 3.0 + 0.003 * (double)i);
                pacmin.push_back(1.1); pdismax.push_back(-7.0); pdismin.push_back(-1.3);
                ts.push_back(0.8 + 0.001 * (double)(i % 5)); tsm.push_back(0.5); etach.push_back(0.93); etadis.push_back(0.91);
            }
            start.push_back((int64_t)ev_cs.size());
        }
        b.n_envs = M; b.n_steps = T; b.timescale = 15; b.n_chargers = C; b.ports_per_charger = npc; b.n_transformers = R; b.horizon = 20;
        b.n_dr_max = 1; b.n_lut = n_lut; b.n_sessions = (int64_t)ev_cs.size();
        b.cs_min_charge_current = imin.data(); b.cs_max_charge_current = imax.data(); b.cs_min_discharge_current = dmin.data();
        b.cs_max_discharge_current = dmax.data(); b.cs_voltage = volt.data(); b.cs_phases = phases.data(); b.cs_transformer = trf.data();
        b.cs_n_ports = topology ? nports.data() : nullptr;
        b.charge_price = b.discharge_price = b.power_setpoints = price.data();
        b.tr_max_power = b.tr_min_power = b.tr_inflexible_load = b.tr_solar_power = b.tr_load_forecast = b.tr_pv_forecast = tr_series.data();
        b.tr_dr = tr_dr.data(); b.tr_n_dr = tr_ndr.data(); b.tr_steps_ahead = tr_ahead.data();
        b.env_session_start = start.data(); b.ev_cs = ev_cs.data(); b.ev_t_arr = ev_ta.data(); b.ev_t_dep = ev_td.data(); b.ev_phases = ev_ph.data();
        b.ev_lut = ev_lut.data(); b.ev_cap0 = cap0.data(); b.ev_B = B.data(); b.ev_desired = des.data(); b.ev_minB = minB.data();
        b.ev_min_emerg = emerg.data(); b.ev_pac_max = pacmax.data(); b.ev_pac_min = pacmin.data(); b.ev_pdis_max = pdismax.data();
        b.ev_pdis_min = pdismin.data(); b.ev_ts = ts.data(); b.ev_tsm = tsm.data(); b.ev_eta_ch = etach.data(); b.ev_eta_dis = etadis.data();
        b.lut = lut.data();
    }
};

static ev2g_config config(int state_kind = EV2G_STATE_V2G_PROFIT_MAX, int flags = 0, int n_active = 0) {
    ev2g_config c{};
    c.state_kind = state_kind; c.flags = flags; c.n_active_envs = n_active;
    return c;
}

// the plan functions in the loader's order; `wave_path` stands for the router's decision
static int make_plan(LoadPlan &p, const ev2g_scenario_batch &b, const ev2g_config &cfg, const LoadSwitches &sw, bool wave_path, std::string &msg) {
    int rc = load_plan_check(p, &b, cfg, msg);
    if (!rc) rc = load_plan_layout(p, &b, cfg, sw, msg);
    if (!rc) rc = load_plan_order(p, &b, msg);
    if (rc) return rc;
    load_plan_constants(p, &b);
    load_plan_records(p, &b);
    load_plan_dictionary(p, wave_path, sw);
    load_plan_big(p, &b, 16);
    return EV2G_OK;
}

static void check_plan(const LoadPlan &p, const ev2g_scenario_batch &b, const ev2g_config &cfg, bool wave_path) {
    const int M = p.M, P = p.P, C = p.C;
    const long long S = p.S, SD = p.SD;
    CHECK(M == b.n_envs && S == b.n_sessions && (int)p.pbase.size() == C + 1 && p.pbase[C] == P);
    // slot_port and port_slot are inverse
    CHECK((int)p.slot_port.size() == P && (int)p.port_slot.size() == P);
    for (int q = 0; q < P; q++) {
        CHECK(p.port_slot[q] >= 0 && p.port_slot[q] < P && p.slot_port[p.port_slot[q]] == q);
        CHECK(p.slot_port[q] >= 0 && p.slot_port[q] < P && p.port_slot[p.slot_port[q]] == q);
        CHECK(p.slot_tr[q] == b.cs_transformer[p.slot_cs[q]] && (q == 0 || p.slot_tr[q - 1] <= p.slot_tr[q]));   // transformer-major
        CHECK(p.slot_port[q] >= p.pbase[p.slot_cs[q]] && p.slot_port[q] < p.pbase[p.slot_cs[q] + 1]);
    }
    // session storage: packed, or fixed-size blocks
    const bool refillable = (cfg.flags & EV2G_FLAG_REFILLABLE) != 0;
    CHECK(SD == (refillable ? p.cap * M : S) && (refillable || p.cap == 0));
    CHECK((long long)p.dev_to_host.size() == SD && (long long)p.host_to_dev.size() == S && (long long)p.sess_port.size() == S);
    long long used = 0;
    for (int m = 0; m < M; m++) {
        const long long n = b.env_session_start[m + 1] - b.env_session_start[m];
        CHECK(p.scn_sess[m] == (refillable ? p.cap * m : b.env_session_start[m]) && p.scn_sess_end[m] == p.scn_sess[m] + n);
        CHECK(!refillable || n <= p.cap);
        for (long long d = p.scn_sess[m]; d < p.scn_sess[m + 1]; d++) {   // used slots first, then the holes
            const long long hs = p.dev_to_host[d];
            if (d < p.scn_sess_end[m]) {
                CHECK(hs >= b.env_session_start[m] && hs < b.env_session_start[m + 1] && p.host_to_dev[hs] == d);
                used++;
            } else
                CHECK(hs == -1);
        }
    }
    CHECK(used == S);
    for (long long s = 0; s < S; s++) CHECK(p.host_to_dev[s] >= 0 && p.host_to_dev[s] < SD && p.dev_to_host[p.host_to_dev[s]] == s);
    // sess_port: a naive replay of the reference's first-free assignment, one busy_until per port
    for (int m = 0; m < M; m++) {
        std::vector<int> busy_until(P, 0);
        for (long long s = b.env_session_start[m]; s < b.env_session_start[m + 1]; s++) {
            int port = p.pbase[b.ev_cs[s]];
            while (busy_until[port] > b.ev_t_arr[s] - 1) port++;
            CHECK(port < p.pbase[b.ev_cs[s] + 1] && p.sess_port[s] == port);
            busy_until[port] = b.ev_t_dep[s];
        }
    }
    // a port's sessions are consecutive in device order and rise in arrival; the chained windows; the per-port tables
    for (int m = 0; m < M; m++) {
        std::vector<int> first(P, -1), end(P, -1);
        for (long long d = p.scn_sess[m]; d < p.scn_sess_end[m]; d++) {
            const long long hs = p.dev_to_host[d];
            const int q = p.ss_slot[d];
            CHECK(q == p.port_slot[p.sess_port[hs]]);
            CHECK(p.ss_tarr[d] == b.ev_t_arr[hs] && p.ss_tdep[d] == b.ev_t_dep[hs] && p.ss_B[d] == b.ev_B[hs] && p.ss_lut[d] == b.ev_lut[hs]);
            const bool chained = d + 1 < p.scn_sess_end[m] && p.ss_slot[d + 1] == q;
            if (d + 1 < p.scn_sess_end[m]) CHECK(p.ss_slot[d + 1] >= q);            // slots in order: each port's run is consecutive
            if (chained) CHECK(p.ss_tarr[d + 1] > p.ss_tdep[d]);                        // ... and rises in arrival
            CHECK(p.ss_ntarr[d] == (chained ? p.ss_tarr[d + 1] : EV2G_INT_MAX) && p.ss_ntdep[d] == (chained ? p.ss_tdep[d + 1] : EV2G_INT_MAX));
            CHECK(p.tails[d].nt_arr == p.ss_ntarr[d] && p.tails[d].nt_dep == p.ss_ntdep[d] && p.tails[d].des == b.ev_desired[hs]);
            if (first[q] < 0) first[q] = (int)d;
            end[q] = (int)d + 1;
        }
        for (int q = 0; q < P; q++) {
            const size_t g = (size_t)m * P + q;
            CHECK(p.port_first[g] == first[q] && p.port_end[g] == end[q]);
            CHECK(p.port_first_win[g].x == (first[q] < 0 ? EV2G_INT_MAX : p.ss_tarr[first[q]]) && p.port_first_win[g].y == (first[q] < 0 ? EV2G_INT_MAX : p.ss_tdep[first[q]]));
        }
    }
    // the records' constants, and the dictionary: entry of every used session, numbered by first occurrence in device order
    int next_entry = 0;
    for (long long d = 0; d < SD; d++) {
        const long long hs = p.dev_to_host[d];
        if (hs < 0) continue;
        const int cs = b.ev_cs[hs];
        const SessRec &r = p.recs[d];
        const double vg = b.cs_voltage[cs] * std::sqrt((double)b.cs_phases[cs]);
        CHECK(r.gate_ch == b.ev_pac_min[hs] * 1000.0 / vg && r.gate_dis == b.ev_pdis_min[hs] * 1000.0 / vg);
        CHECK(r.v == b.cs_voltage[cs] * std::sqrt((double)std::min(b.cs_phases[cs], b.ev_phases[hs])) && r.rB == 1.0 / r.B && r.rv == 1.0 / r.v);
        CHECK(r.potc == r.v * std::min(r.pacmax * 1000.0 / r.v, b.cs_max_charge_current[cs]) / 1000.0);
        CHECK(p.ss_afap[d] == p.sess_afap_host[hs] && p.ss_afap[d] <= b.ev_B[hs] && p.ss_afap[d] >= b.ev_cap0[hs]);
        if (!wave_path) continue;
        const int k = p.dyns[d].cls;
        CHECK(k >= 0 && (size_t)k < p.cls_tab.size());
        const ClsRec want = ev2g_cls_of(r);
        CHECK(std::memcmp(&want, &p.cls_tab[k], sizeof(ClsRec)) == 0);
        CHECK(p.dyns[d].ts == b.ev_ts[hs] && p.dyns[d].lut == b.ev_lut[hs] && p.dyns[d].eta_ch == b.ev_eta_ch[hs] && p.dyns[d].eta_dis == b.ev_eta_dis[hs]);
        if (p.dict) { CHECK(k <= next_entry); if (k == next_entry) next_entry++; }
        else CHECK(k == (int)d);
    }
    if (wave_path && p.dict) CHECK(p.cls_tab.size() == EV2G_CLS_CAP && (int)p.cls_map.size() == next_entry);
    if (wave_path && !p.dict) CHECK(p.cls_map.empty() && (long long)p.cls_tab.size() == std::max<long long>(SD, 1));
}

// plans `batch`, expects success and checks the plan
static LoadPlan good(const char *name, const Batch &batch, const ev2g_config &cfg = config(), const LoadSwitches &sw = LoadSwitches{}, bool wave_path = true) {
    g_case = name;
    LoadPlan p;
    std::string msg;
    const int rc = make_plan(p, batch.b, cfg, sw, wave_path, msg);
    if (rc) std::fprintf(stderr, "[%s] refused: %s\n", name, msg.c_str());
    CHECK(rc == EV2G_OK);
    check_plan(p, batch.b, cfg, wave_path);
    return p;
}

// plans `b`, expects the refusal `want`
static void refused(const char *name, const ev2g_scenario_batch &b, const char *want, const ev2g_config &cfg = config(), const LoadSwitches &sw = LoadSwitches{}) {
    g_case = name;
    LoadPlan p;
    std::string msg;
    const int rc = make_plan(p, b, cfg, sw, true, msg);
    if (rc != EV2G_ERR_ARG || msg != want) std::fprintf(stderr, "[%s] code %d, message: %s\n", name, rc, msg.c_str());
    CHECK(rc == EV2G_ERR_ARG && msg == want);
}

static const std::vector<Charger> kTwo = {{0, 1, 3}, {0, 1, 3}};

static void fixed_cases() {
    good("one scenario, two ports", Batch(8, 1, kTwo, {{{0, 1, 3, 0, 3}, {1, 2, 5, 1, 1}, {0, 4, 6, 0, 3}}}));
    good("two scenarios, two ports", Batch(8, 1, kTwo, {{{1, 1, 3, 0, 3}, {0, 2, 5, 1, 1}}, {{0, 1, 1, 2, 2}, {0, 2, 2, 2, 2}, {1, 2, 8, 0, 3}}}));
    {   // a 2-port charger: the second car arrives while the first is parked (port 1), the third right after the first left (port 0 again)
        const LoadPlan p = good("first-free replay", Batch(12, 1, {{0, 2, 3}}, {{{0, 1, 4, 0, 3}, {0, 2, 9, 1, 3}, {0, 5, 7, 2, 3}}}));
        CHECK((p.sess_port == std::vector<int>{0, 1, 0}) && (p.host_to_dev == std::vector<int>{0, 2, 1}));
        CHECK(p.ss_ntarr[0] == 5 && p.ss_ntdep[0] == 7 && p.ss_ntarr[1] == EV2G_INT_MAX && p.ss_ntarr[2] == EV2G_INT_MAX);
    }
    {   // two transformers, chargers interleaved: slot order differs from port order
        const Batch bt(8, 2, {{0, 1, 3}, {1, 1, 1}, {0, 1, 3}, {1, 1, 3}}, {{{1, 1, 2, 0, 3}, {2, 1, 3, 1, 3}, {0, 2, 4, 0, 1}, {3, 3, 5, 2, 3}, {1, 3, 6, 1, 2}}});
        for (int sk = 0; sk < 3; sk++) {
            const LoadPlan p = good("two transformers", bt, config(sk), LoadSwitches{}, false);
            CHECK((p.slot_port == std::vector<int>{0, 2, 1, 3}) && (p.tr_seg == std::vector<int>{0, 2, 4}) && p.max_seg == 2);
            CHECK(p.D == (sk == EV2G_STATE_PUBLIC_PST ? 15 : sk == EV2G_STATE_V2G_PROFIT_MAX ? 30 : 110));
            if (sk == EV2G_STATE_V2G_PROFIT_MAX_LOADS) CHECK((p.tr_obs == std::vector<int>{22, 66}) && (p.slot_obs == std::vector<int>{62, 64, 106, 108}));
        }
    }
    {   // a topology with port counts 3, 2, 1; in rising order the reference's action mask leaves its array
        const std::vector<std::vector<Sess>> ss = {{{0, 1, 6, 0, 3}, {0, 1, 2, 1, 3}, {1, 2, 4, 2, 3}, {0, 3, 8, 0, 1}, {2, 3, 3, 1, 3}, {0, 3, 5, 2, 3}, {1, 5, 8, 0, 3}}};
        const LoadPlan p = good("topology 3,2,1", Batch(8, 1, {{0, 3, 3}, {0, 2, 3}, {0, 1, 1}}, ss, true), config(EV2G_STATE_PUBLIC_PST), LoadSwitches{}, false);
        CHECK(p.het && p.P == 6 && (p.pbase == std::vector<int>{0, 3, 5, 6}) && (p.slot_mask == std::vector<int>{0, 1, 2, 2, 3, 2}));
        CHECK((p.sess_port == std::vector<int>{0, 1, 3, 1, 5, 2, 3}));
        refused("topology 1,2,3", Batch(8, 1, {{0, 1, 1}, {0, 2, 3}, {0, 3, 3}}, {{}}, true).b,
                "ev2g_load_scenarios: this charger order makes the reference's action mask index i*n_ports+j leave the mask array "
                "(ev2gym_env.py:457 raises IndexError); order the chargers by falling port count");
    }
    {   // a refillable pool with unequal session counts: fixed-size blocks with holes; EV2G_POOL_SESSION_CAP raises the block size
        const Batch bt(8, 1, kTwo, {{{0, 1, 3, 0, 3}, {1, 2, 5, 1, 1}, {0, 4, 6, 0, 3}}, {}, {{1, 3, 3, 2, 2}}});
        LoadPlan p = good("refillable pool", bt, config(EV2G_STATE_V2G_PROFIT_MAX, EV2G_FLAG_REFILLABLE));
        CHECK(p.cap == 16 && p.SD == 48 && p.dev_to_host[3] == -1 && p.dev_to_host[16] == -1 && p.dev_to_host[32] == 3);
        LoadSwitches sw;
        sw.pool_session_cap = 40;
        p = good("refillable pool, raised capacity", bt, config(EV2G_STATE_V2G_PROFIT_MAX, EV2G_FLAG_REFILLABLE), sw);
        CHECK(p.cap == 40 && p.SD == 120);
        sw.pool_session_cap = 8;
        CHECK(good("refillable pool, low capacity", bt, config(EV2G_STATE_V2G_PROFIT_MAX, EV2G_FLAG_REFILLABLE), sw).cap == 16);
        sw.no_dict = true;
        p = good("refillable pool, no dictionary", bt, config(EV2G_STATE_V2G_PROFIT_MAX, EV2G_FLAG_REFILLABLE), sw);
        CHECK(!p.dict && p.cls_tab.size() == 48);
    }
    good("a scenario without sessions", Batch(8, 1, kTwo, {{}, {{0, 1, 2, 0, 3}}, {}}));
    good("no sessions at all", Batch(8, 1, kTwo, {{}}));
    good("fewer envs than scenarios", Batch(8, 1, kTwo, {{}, {{0, 1, 2, 0, 3}}, {}}), config(EV2G_STATE_V2G_PROFIT_MAX, 0, 2));
    {   // more distinct operand tuples than the dictionary holds: one entry per session
        std::vector<Sess> ss;
        for (int i = 0; i < EV2G_CLS_CAP + 1; i++) ss.push_back({i % 2, 1 + i / 2, 1 + i / 2, -1, 3});
        const LoadPlan p = good("dictionary overflow", Batch(2100, 1, kTwo, {ss}));
        CHECK(!p.dict && p.cls_tab.size() == EV2G_CLS_CAP + 1);
        ss.pop_back();
        CHECK(good("dictionary exactly full", Batch(2100, 1, kTwo, {ss})).dict);
    }
    {   // ev2g_step_big's classes: 17 distinct charger tuples are one too many
        std::vector<Charger> cs(17, Charger{0, 1, 3});
        Batch bt(8, 1, cs, {{{16, 1, 3, 0, 3}, {3, 2, 9, 1, 3}}});
        for (int c = 0; c < 17; c++) bt.imin[c] = 6.0 + 0.1 * c;
        LoadPlan p = good("seventeen charger classes", bt);
        CHECK(p.many && p.tmax == 9 && p.tmin == 0 && p.even);
        bt.imin[16] = bt.imin[3];
        p = good("sixteen charger classes", bt);
        CHECK(!p.many && p.ctab.size() == 16 * 6 && p.ccls[16] == 3 && p.ccls[15] == 15 && p.ptab[0] == p.recs[0].potc);
    }
}

static void refusals() {
    const std::vector<std::vector<Sess>> one = {{{0, 1, 3, 0, 3}, {1, 2, 5, 1, 1}}};
    auto with = [&](auto change) { Batch bt(8, 1, kTwo, one); change(bt); return bt; };
    refused("n_active_envs", Batch(8, 1, kTwo, one).b, "ev2g_load_scenarios: n_active_envs exceeds the number of scenarios in the batch", config(0, 0, 2));
    for (int k = 0; k < 6; k++)
        refused("non-positive size", with([&](Batch &t) { int32_t *f[6] = {&t.b.n_envs, &t.b.n_steps, &t.b.n_chargers, &t.b.ports_per_charger, &t.b.n_transformers, &t.b.timescale}; *f[k] = 0; }).b,
                "ev2g_load_scenarios: non-positive size");
    refused("horizon", with([](Batch &t) { t.b.horizon = 10; }).b, "ev2g_load_scenarios: horizon must be 20 (state.py:119,129-132)");
    refused("ports per charger", with([](Batch &t) { t.b.ports_per_charger = 33; }).b, "ev2g_load_scenarios: more than 32 ports per charger unsupported");
    refused("cs_n_ports < 1", with([](Batch &t) { t.nports[1] = 0; t.b.cs_n_ports = t.nports.data(); }).b, "ev2g_load_scenarios: cs_n_ports must be >= 1");
    refused("ports_per_charger not the maximum", with([](Batch &t) { t.b.cs_n_ports = t.nports.data(); t.b.ports_per_charger = 2; }).b,
            "ev2g_load_scenarios: ports_per_charger must be the maximum of cs_n_ports");
    refused("n_sessions", with([](Batch &t) { t.b.n_sessions = 3; }).b, "ev2g_load_scenarios: env_session_start inconsistent with n_sessions");
    refused("env_session_start[0]", with([](Batch &t) { t.start[0] = 1; }).b, "ev2g_load_scenarios: env_session_start inconsistent with n_sessions");
    refused("too many sessions", with([](Batch &t) { t.start[1] = t.b.n_sessions = 0x7ffffff1LL; }).b, "ev2g_load_scenarios: too many sessions for 32-bit indices");
    {
        Batch bt(8, 1, kTwo, std::vector<std::vector<Sess>>(1000));
        bt.b.n_steps = 65535; bt.b.n_transformers = 50;   // (refused before any [M,R,T] array is read)
        refused("32-bit element offsets", bt.b, "ev2g_load_scenarios: batch too large for 32-bit element offsets "
                                                "(need M*P, M*D, M*R*(T+1)*40, T*M*C < 2^31): split it over more handles / GPUs");
    }
    const char *k16 = "ev2g_load_scenarios: simulation_length and the number of efficiency tables must stay below 65536 (a port's state line "
                      "packs charging_cycles and the table id into 16 bits each)";
    refused("simulation_length", with([](Batch &t) { t.b.n_steps = 65536; }).b, k16);
    refused("n_lut", with([](Batch &t) { t.b.n_lut = 65535; }).b, k16);
    refused("cs_transformer", with([](Batch &t) { t.trf[1] = 1; }).b, "ev2g_load_scenarios: cs_transformer out of range");
    refused("cs_transformer < 0", with([](Batch &t) { t.trf[0] = -1; }).b, "ev2g_load_scenarios: cs_transformer out of range");
    refused("cs_phases", with([](Batch &t) { t.phases[1] = 4; }).b, "ev2g_load_scenarios: cs_phases must be 1..3");
    {
        LoadSwitches sw;
        sw.pool_session_cap = 0x40000000LL;
        Batch bt(8, 1, kTwo, {{}, {}});
        refused("refillable slots", bt.b, "ev2g_load_scenarios: too many session slots for 32-bit indices (refillable pool)", config(0, EV2G_FLAG_REFILLABLE), sw);
    }
    {
        Batch bt(8, 1, kTwo, {{}, {}});
        bt.start[1] = -1;
        refused("env_session_start not monotone", bt.b, "ev2g_load_scenarios: env_session_start not monotone");
    }
    refused("ev_cs", with([](Batch &t) { t.ev_cs[1] = 2; }).b, "ev2g_load_scenarios: ev_cs out of range");
    refused("ev_cs < 0", with([](Batch &t) { t.ev_cs[0] = -1; }).b, "ev2g_load_scenarios: ev_cs out of range");
    refused("t_arr < 1", with([](Batch &t) { t.ev_ta[0] = 0; }).b, "ev2g_load_scenarios: need 1 <= t_arr <= t_dep");
    refused("t_dep < t_arr", with([](Batch &t) { t.ev_td[1] = 1; }).b, "ev2g_load_scenarios: need 1 <= t_arr <= t_dep");
    refused("arrival order", with([](Batch &t) { t.ev_ta[0] = 3; }).b, "ev2g_load_scenarios: sessions must be sorted by arrival");
    refused("ev_phases", with([](Batch &t) { t.ev_ph[1] = 0; }).b, "ev2g_load_scenarios: ev_phases must be 1..3");
    refused("ev_lut", with([](Batch &t) { t.ev_lut[0] = 0; }).b, "ev2g_load_scenarios: ev_lut out of range");
    refused("no free port", with([](Batch &t) { t.ev_cs[1] = 0; }).b,
            "ev2g_load_scenarios: no free port for a session (assert n_evs_connected < n_ports, ev_charger.py:271)");
    refused("no free port at t_dep", with([](Batch &t) { t.ev_cs[1] = 0; t.ev_ta[1] = 3; }).b,
            "ev2g_load_scenarios: no free port for a session (assert n_evs_connected < n_ports, ev_charger.py:271)");
    // two faults: the earlier check reports
    refused("horizon before cs_phases", with([](Batch &t) { t.b.horizon = 10; t.phases[0] = 0; }).b, "ev2g_load_scenarios: horizon must be 20 (state.py:119,129-132)");
    refused("cs_transformer before ev_cs", with([](Batch &t) { t.trf[1] = 1; t.ev_cs[0] = 7; }).b, "ev2g_load_scenarios: cs_transformer out of range");
    refused("ev_cs before t_arr (same session)", with([](Batch &t) { t.ev_cs[0] = 7; t.ev_ta[0] = 0; }).b, "ev2g_load_scenarios: ev_cs out of range");
    refused("the first session's fault", with([](Batch &t) { t.ev_ph[0] = 0; t.ev_cs[1] = 7; }).b, "ev2g_load_scenarios: ev_phases must be 1..3");
}

// 200 batches from a fixed LCG: P <= 8, T <= 24, arrivals sorted, never more parked cars on a charger than it has ports
static void random_family() {
    uint64_t x = 0x2545F4914F6CDD1Dull;
    auto rnd = [&](int n) { x = x * 6364136223846793005ull + 1442695040888963407ull; return (int)((x >> 33) % (uint64_t)n); };
    for (int it = 0; it < 200; it++) {
        const int R = 1 + rnd(2), T = 4 + rnd(21), M = 1 + rnd(3);
        const bool topology = rnd(3) == 0;
        const int uniform = 1 + rnd(2);
        std::vector<Charger> cs;
        int P = 0;
        while (cs.size() < 4 && (cs.empty() || rnd(4) != 0)) {
            int np = topology ? 1 + rnd(3) : uniform;
            if (topology && !cs.empty()) np = std::min(np, cs.back().ports);   // falling port counts
            if (P + np > 8) break;
            cs.push_back({rnd(R), np, 1 + rnd(3)});
            P += np;
        }
        std::vector<std::vector<Sess>> scn(M);
        for (auto &ss : scn) {
            if (rnd(6) == 0) continue;   // a scenario without sessions
            std::vector<std::vector<int>> parked_until(cs.size());
            for (int t = 1; t <= T; t++)
                for (int k = rnd(3); k > 0; k--) {
                    const int c = rnd((int)cs.size());
                    auto &pu = parked_until[c];
                    pu.erase(std::remove_if(pu.begin(), pu.end(), [&](int td) { return td < t; }), pu.end());
                    if ((int)pu.size() >= cs[c].ports) continue;
                    const int td = t + rnd(6);
                    pu.push_back(td);
                    ss.push_back({c, t, td, rnd(4), 1 + rnd(3)});
                }
        }
        const int n_lut = rnd(3);
        const Batch bt(T, R, cs, scn, topology, n_lut);
        LoadSwitches sw;
        sw.no_dict = rnd(4) == 0;
        char name[64];
        std::snprintf(name, sizeof name, "random batch %d", it);
        const int sk = rnd(3), flags = rnd(2) ? EV2G_FLAG_REFILLABLE : 0, n_active = rnd(2) ? 1 + rnd(M) : 0;
        const bool wave_path = rnd(4) != 0;
        good(name, bt, config(sk, flags, n_active), sw, wave_path);
    }
}

int main() {
    fixed_cases();
    refusals();
    random_family();
    std::puts("load_plan_check: ok");
    return 0;
}
