// The body of ONE step of ev2g_step_wave (ev2g_step_wave.h), included there inside each of the kernel's step loops -- not a header of its own.
// The including scope defines the compile-time OUT (this step writes the observation / reward / done / mask rows), the step's index kk in the launch,
// EV2G_STEP_SKIP(n) (a fast-forward pass did n steps: on to step kk + n) and EV2G_STEP_BREAK (the launch ends here).  Everything else is the kernel's own scope.
#if defined(EV2G_PHASE_TIMING) && defined(EV2G_PT_OUTER)
        PT_MARK(5)
#elif defined(EV2G_PT_DRAIN)     // (tools/phase_timing.py -DEV2G_PT_DRAIN=1: slot 7 := a wait for the step before's stores and nothing else, the step-end bookkeeping counts as phase E; =0: the same two marks without the wait)
        PT_MARK(5)
        if (EV2G_PT_DRAIN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PT_MARK(7)
#elif !defined(EV2G_PT_BSPLIT)   // (tools/phase_timing.py -DEV2G_PT_BSPLIT: slot 7 := the battery maths' operand wait, the loop top counts as phase A)
        PT_MARK(7)
#endif
        asm volatile("" : "+s"(S));
        int tid_l = tid, g_l = g, e_l = e, q_l = q, lane_l = lane;
        asm volatile("" : "+v"(tid_l), "+v"(g_l), "+v"(e_l), "+v"(q_l), "+v"(lane_l));
        const unsigned g8 = (unsigned)g_l * 8u;   // byte offset of this port in every [E*P] float64 / int2 array
        if (!FULL && t >= T) {  // episode finished inside a fused run: in-kernel ev2g_reset for this workgroup
            if (!auto_reset) EV2G_STEP_BREAK;
            off = ev2g_scn(off, io.scn_stride, M);
            if (valid) {
                const unsigned gs8 = (unsigned)(ev2g_scn(e_l, off, M) * P + q_l) * 8u;   // this port in the scenario pool
                const i2v w = ldg32<i2v>(S->port_first_win, gs8);
                s_ta[tid_l] = w.x; s_td[tid_l] = w.y; s_ss[tid_l] = ldg32<int>(S->port_first, gs8 >> 1); s_cyc[tid_l] = 0;
                s_cap[tid_l] = 0.0; s_tot[tid_l] = 0.0; s_prev[tid_l] = 0.0; s_abse[tid_l] = 0.0; s_dirty[tid_l] = 3;
                stg32<double>(PA(EV2G_PS_PENERGY), g8, 0.0);
                stg32<double>(PA(EV2G_PS_PCURRENT), g8, 0.0);
                stg32<double>(PA(EV2G_PS_SATSUM), g8, 0.0);   // single-port chargers: charger index == port index
                stg32<int>(PA(EV2G_PS_SERVED), g8 >> 1, 0);
                if (log_cs) {   // single-port chargers: charger index == port index
                    stg32<double>(S->cs_profits, g8, 0.0); stg32<double>(S->cs_e_ch, g8, 0.0); stg32<double>(S->cs_e_dis, g8, 0.0);
                }
            }
            if (head) {
                for (int i = 0; i < 8; i++) stg32<double>(env_acc, (unsigned)e_l * 64u + (unsigned)i * 8u, 0.0);
                for (int i = 0; i < 7; i++) eacc[elg * 7 + i] = 0.0;
            }
            t = 0;
        }
        double *obs = F64 ? obs_run : ((!FULL && io.obs) ? io.obs + (long long)kk * io.o_stride : nullptr);       // uniform bases (scalar arithmetic)
        float *obs32 = F32 ? obs32_run : ((!FULL && S->x_obs32) ? (float *)S->x_obs32 + (long long)(io.step0 + kk) * S->x_o32_stride : nullptr);
        uint8_t *mask = FULL ? mask_run : (io.mask ? io.mask + (long long)kk * io.m_stride : nullptr);
        const int sstep = t + 1;
        const bool last_step = LSO ? OUT : ((kk == k_steps - 1) || (!FULL && sstep >= T && !auto_reset));   // (LSO: the peeled step is the launch's last by construction)
        constexpr bool out = OUT;   // this step's observation / reward / done / mask rows are written
        int *cntk = cnt + 2 * (kk & 1);
        // next step's counters, cleared BEFORE this step's first barrier: they were last read in the battery-maths phase of the step
        // before, which a busy step closes with a barrier and a quiet step leaves at zero
        if (tid_l < 2) cnt[2 * ((kk + 1) & 1) + tid_l] = 0;

        double a_cur = a_next;   // this step's action; the prefetch below replaces a_next by the next step's
        if (ACT) {
            // ---- the policy, on the 16 observation rows of this workgroup's envs (ev2g_mlp3_inline, ev2g_mlp.h) ----
            if (NWF > 1)
                ev2g_mlp3_inline_f32<FKS1, 25, 19, FNT3, BLOCK / 64, EV2G_FUSED_RINGF>(fa.m, bufXf, FSXF, bufH1, bufH1 + 3 * 16 * MC::SH1, (uint16_t *)bufXf, (uint16_t *)(stage + 5 * RS), RS * 4, act_lds, ACT_AS, act_out, min(16, E - e0), tid_l);
            else
            ev2g_mlp3_inline<FKS1, 25, 19, FNT3, BLOCK / 64, (AE == 1 ? EV2G_FUSED_RING : EV2G_FUSED_RING2), AE>(fa.m, bufX, bufH1, bufH2, lbias, act_lds, ACT_AS, act_out, min(16 * AE, E - e0), tid_l);   // (starts and ends with a barrier: the actions are in LDS)
            act_out += io.a_stride;
            a_cur = valid ? (double)act_lds[arow * ACT_AS + q_l] : 0.0;
            // the staging slots of idle lanes must read as +0.0 in the per-env reduction (the lanes behind an env's last port never write them)
            if (!valid) {
#pragma unroll
                for (int k = 0; k < EV2G_NQ; k++) stage[k * RS + tid_l] = 0.0;
            }
            PT_MARK(7)   // (phase-timing builds: slot 7 = the policy, including the wait at its first barrier)
        }
        // ---- prefetch what the rest of this step needs (collected before the stores of phase C) ----
        // Every prefetch is ONE unconditional load from a clamped (always valid) address; the conditions are applied
        // where the value is consumed.  A load inside a divergent branch whose result merges with a default makes the
        // compiler serialise on the destination register (write-after-write) with a full vmcnt(0) drain.
        const bool more = LSO ? !OUT : ((kk + 1 < k_steps) && (FULL || sstep < T || auto_reset));
        const int ec = valid ? e_l : e0;   // clamped env for idle lanes
        const int gc = valid ? g_l : e0 * P;
        if (ACT) {
        } else if (F64) {   // a running pointer instead of a 64-bit scalar product per step
            a_next = ldg32_nt<double>(act_run + (more ? io.a_stride : 0), (unsigned)gc * 8u);
            act_run += io.a_stride;
        } else if (F32) {
            a_next = (double)ldg32_nt<float>(act32_run + (more ? io.a_stride : 0), (unsigned)gc * 4u);
            act32_run += io.a_stride;
        } else
        a_next = IO32 ? (double)ldg32_nt<float>(io.act32 + (long long)(io.step0 + (more ? kk + 1 : kk)) * io.a_stride, (unsigned)gc * 4u)
                      : ldg32_nt<double>(io.actions + (long long)(more ? kk + 1 : kk) * io.a_stride, (unsigned)gc * 8u);
        const int scn = ev2g_scn(ec, off, M);             // this env's scenario in the resident pool
        const unsigned eT64 = FULL ? hb_step : (unsigned)(scn * T) * 64u;  // its rows in the [M,T,8] step table
        const unsigned et64 = eT64 + (unsigned)t * 64u;
        const d2v st0 = ldg32_nt<d2v>(S->step_tab, et64);                                  // charge price, discharge price
        double pf_pch = st0.x, pf_pdis = st0.y;
        // the transformer scalars only the head lane needs: ONE more load in which the head lane (q == 0) takes
        // {inflexible + solar, max_power} and its neighbour takes {min_power, setpoint}; the head lane picks the
        // neighbour's pair up with a DPP wave shift in phase E
        d2v pf_tr = ldg32_nt<d2v>(S->step_tab, et64 + ((q_l == 0) ? 16u : 32u));
        // observation head columns of this env, distributed over its P lanes as 16-byte column PAIRS: pair q, q+P
        double pf_ob0 = 0.0;
        d2v pf_h0 = {0.0, 0.0}, pf_h1 = {0.0, 0.0};
        constexpr int NHEAD = (SK == 1) ? 0 : (SK == 0 ? 60 : 20);   // 20 prices (+ 40 window columns)
        constexpr int NPAIR = NHEAD / 2;
        // (LSO: a step that writes no observation requests none of this)
        if (!out) {
        } else if (SK == 1) {
            pf_ob0 = ldg32_nt<double>(S->step_tab, eT64 + (unsigned)min(sstep, T - 1) * 64u + 40u);   // next setpoint; head lane only, masked by sstep < T
        } else {
            // observation head table [E, T+1, NHEAD]: |charge price| window (zero-padded) + load/PV/limit window, exactly
            // the values of columns 2..2+NHEAD of the observation emitted at the end of step sstep-1 (state.py:65-83, :108-135)
            const unsigned h8 = FULL ? hb_head + (unsigned)sstep * (unsigned)(NHEAD * 8) : (unsigned)((scn * (T + 1) + sstep) * NHEAD) * 8u;
            pf_h0 = ldg32_nt<d2v>(S->head_tab, h8 + (unsigned)min(q_l, NPAIR - 1) * 16u);
            if (!WIDE && P < NPAIR) pf_h1 = ldg32_nt<d2v>(S->head_tab, h8 + (unsigned)min(q_l + P, NPAIR - 1) * 16u);   // (uniform)
        }
        // ---------------- A: home lanes, charger level (ev_charger.py:137-186) ----------------
        bool occ = false;
        double cap_before = 0.0;
        int ta_a = EV2G_INT_MAX, td_a = -1;   // this port's window as phase A saw it (idle lanes: no event)
        // A wavefront none of whose ports holds an EV in this step or receives one at its end (workplace nights, early mornings: a third of the
        // wavefront-steps at cfg2) has nothing to decide in phases A and C: every action is masked, every per-port observation column and mask entry
        // is zero, nothing is staged (phase D skips such a wavefront already).  The full kernels know it from the windows in their registers.
        // (one env per wavefront only: with two or three a wavefront is rarely empty and the test costs more than it saves -- cfg3 +0.8 %, cfg2 -3 %,
        // profiles/r05_ab_empty_wavefront_path.txt)
        const bool wave_live = !FULL || EPW != 1 || __ballot(valid && ((r_ta <= t && t <= r_td) || r_ta == sstep)) != 0ull;   // (uniform)
        if (FFW && !OUT) asm volatile("" : "+v"(ff_lim_v), "+v"(ff_next_v));
        // (EPW first: a scalar the loop holds anyway -- with several envs per wavefront, cfg3, the path costs a scalar compare and no vector instruction)
        // (the launch's last step never fast-forwards and nobody reads what it would tell the other wavefronts: none of the path is in the OUT body)
        if (FFW && !OUT && EPW == 1 && __builtin_amdgcn_readfirstlane(ff_lim_v) != 0) {   // (uniform) how long this wavefront's env stays EV-free, for the other wavefronts (read behind the barrier below)
            int ff_next = __builtin_amdgcn_readfirstlane(ff_next_v);
            if (wave_live) ff_next = t;
            else if (ff_next <= t) {   // the first EV-free step behind a live one (or of the launch): the env wakes in the step at whose end its
                                       // earliest EV arrives (sstep == r_ta); idle lanes and wavefronts without an env never constrain
                int m = (valid && r_ta > sstep) ? r_ta : EV2G_INT_MAX;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
                ff_next = __builtin_amdgcn_readfirstlane(m) - 1;
            }
            ff_next_v = ff_next;
            if (lane_l == 0) ffx[4 * (kk & 1) + (tid_l >> 6)] = (unsigned short)min(ff_next - t, 0xffff);
        }
        if (valid && wave_live) {
            // every LDS operand of the phase in one batch (one wait) instead of one round trip per branch
            int ta = FULL ? r_ta : s_ta[tid_l], td = FULL ? r_td : s_td[tid_l];
            double cap_b = s_cap[tid_l], c_thr = s_cst[0 * 64 + q_l], c_dmin = s_cst[1 * 64 + q_l];
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ta), "+v"(td), "+v"(cap_b), "+v"(c_thr), "+v"(c_dmin));
            ta_a = ta; td_a = td;
            occ = (ta <= t) && (t <= td);
            if (log_soc && occ) cap_before = cap_b;
            double a = occ ? a_cur : 0.0;
            // one port per charger: a / sum(a) = a / a, which is exactly +-1 for every finite action (ev_charger.py:143-149)
            a = (a > 1.0) ? 1.0 : ((a < -1.0) ? -1.0 : a);
            // Straight-line selects instead of nested branches (each divergent `if` is three scalar instructions around a handful of vector
            // ones): an empty port has a == 0, hence x == 0 and amps == 0, like the branch it replaces.  |a| <= 1, so rint(a * 1e5) is
            // within the range in which the two-FMA form of the division by 1e5 is exact (div_int_by_const, tests/test_fma_division.py):
            // no fallback division.
            const double n5 = rint(a * 100000.0), q5 = n5 * (1.0 / 100000.0);
            const double x = fma(fma(-q5, 100000.0, n5), 1.0 / 100000.0, q5);   // rnd5 (ev_charger.py:157)
            const double ac = x * c_imax, ad = x * c_dmaxabs;
            const double amps_c = (ac < c_thr) ? 0.0 : ac, amps_d = (ad > c_dmin - 0.01) ? c_dmin : ad;
            const double amps = (x > 0.0) ? amps_c : ((x < 0.0) ? amps_d : 0.0);
            s_amps[tid_l] = amps;
            stage[0 * RS + tid_l] = 0.0;
            stage[4 * RS + tid_l] = 0.0;
            stage[5 * RS + tid_l] = 0.0;
            stage[6 * RS + tid_l] = 0.0;
            stage[7 * RS + tid_l] = 0.0;
            if (amps != 0.0) items[(amps > 0.0) ? atomicAdd(&cntk[0], 1) : NS - 1 - atomicAdd(&cntk[1], 1)] = tid_l;
        }
        PT_MARK(0)
        // Departures and arrivals are known before the step (occupancy does not depend on the actions): the fields phase C needs
        // from the session record -- its last four 16-byte chunks -- travel with the other prefetches instead of being fetched,
        // dependently, inside that phase's branches.  Only wavefront-steps that have such an event issue them (about half at cfg2);
        // the other lanes of such a wavefront read record 0.
        const bool ev_dep = occ && t >= td_a, ev_arr = (ta_a == sstep);
        d2v pf_c2 = {0.0, 0.0}, pf_c7 = {0.0, 0.0};   // an arrival: {B, RN(1/B)}, {cap0, potc} of the arriving session's record ...
        d2v pf_d0 = {1.0, 1.0};                       // ... and its SessDyn: {transition_soc, charge efficiency},
        i4v pf_d1 = {0, 0, -1, 0};                    //     {discharge efficiency, efficiency-table id, dictionary entry}
        i4v pf_tl = {0, 0, 0, 0};                     // a departure: {des (two words), next window} of the leaving session's tail entry
        if (__ballot(ev_dep || ev_arr) != 0ull) {   // (uniform)
            const unsigned sse = (ev_dep || ev_arr) ? (unsigned)s_ss[tid_l] : 0u;
            static_assert(offsetof(SessRec, B) == 40 && offsetof(SessRec, rB) == 48 && offsetof(SessRec, cap0) == 112 && offsetof(SessRec, potc) == 120 && sizeof(SessTail) == 16 &&
                          offsetof(SessTail, nt_arr) == 8, "SessRec / SessTail layout");
            pf_c2 = ldg32<d2v_a8>(S->rec, sse * (unsigned)sizeof(SessRec) + 40u); pf_c7 = ldg32<d2v>(S->rec, sse * (unsigned)sizeof(SessRec) + 112u);
            pf_tl = ldg32<i4v>(S->tail, sse * 16u);
            pf_d0 = ldg32<d2v>(S->sess_dyn, sse * 32u); pf_d1 = ldg32<i4v>(S->sess_dyn, sse * 32u + 16u);
        }
#if defined(EV2G_PHASE_TIMING) && defined(EV2G_PT_OUTER)
        PT_MARK(0)
#else
        PT_MARK(6)
#endif
        lds_barrier();
        PT_MARK(1)

        // ---------------- B: worker lanes, battery maths on the compact list ----------------
        // The wavefronts that hold list items are the critical path of the whole workgroup (the others wait at the next
        // barrier): they issue at raised priority until their items are done.
        const int nch = cntk[0], ndis = cntk[1];
        // A step in which no port of the workgroup has an EV to integrate (the night half of a workplace episode, the early morning: 40 % of the
        // workgroup-steps at cfg2) has no battery-maths phase to fence: the second barrier is skipped.  Every wavefront reads the same counts.
        if (nch + ndis != 0) {
        __builtin_amdgcn_s_setprio(3);
        {
            const int nchp = (nch + 63) & ~63;
            for (int i = tid_l; i < nchp + ndis; i += BLOCK) {
                int h = -1;
                if (i < nch) h = items[i];
                else if (i >= nchp) h = items[NS - 1 - (i - nchp)];
                if (h >= 0) {
                    const double amps_h = s_amps[h];
                    const int dw_h = s_dirty[h];
                    const int lut_id = ((dw_h >> 8) & LUTMASK) - 1;
                    // table entry and session record are independent loads: one memory round trip, not two.  The look-up
                    // is unconditional (clamped index); whether it applies is decided where it is used.
                    const int li = (lut_id >= 0) ? ev_lut_index(lut_id, amps_h) : -1;
                    double lut_raw = ldg32<double>(S->lut, (unsigned)max(li, 0) * 8u);
                    // full kernels: the operands of the car model from the dictionary (an L1 hit), transition_soc / efficiency from LDS
                    const unsigned r8 = ((FULL && wa.dict) ? (unsigned)dw_h >> 20 : (unsigned)s_ss[h]) * (unsigned)sizeof(SessRec);
                    const double cap0 = s_cap[h], prev0 = s_prev[h];
                    const int cyc0 = s_cyc[h];
                    EvRes o;
                    if (i < nchp) {   // (uniform: the discharge items start on a wavefront boundary)
                        SessRec r;
                        if (FULL) { const double ts_h = s_ts[h], eta_h = s_etac[h]; r = ldg32_cls_charge(S->cls_rec, r8); r.ts = ts_h; r.eta_ch = eta_h; }
                        else r = ldg32_rec_charge(S->rec, r8);
                        asm volatile("" : "+v"(lut_raw));
#if defined(EV2G_PHASE_TIMING) && defined(EV2G_PT_BSPLIT)
                        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                        PT_MARK(7)
#endif
                        const double lutv = (li >= 0) ? lut_raw : 1.0 / 100.0;
                        o = ev_math_charge(r, lutv, amps_h, cap0, prev0, s_tot[h], cyc0, sixty_over_dt, dt_over_60, pow2_dt, lut_id >= 0);
                    } else {
                        SessRec r;
                        if (FULL) { const double eta_h = s_etad[h]; r = ldg32_cls_discharge(S->cls_rec, r8); r.eta_dis = eta_h; }
                        else r = ldg32_rec_discharge(S->rec, r8);
                        asm volatile("" : "+v"(lut_raw));
                        const double lutv = (li >= 0) ? lut_raw : 1.0 / 100.0;
                        o = ev_math_discharge(r, lutv, amps_h, cap0, prev0, s_tot[h], cyc0, dtd, lut_id >= 0, S->rdt, S->dt_fdiv != 0);   // (fetched here, by the discharging wavefronts only: not kept across the step loop)
                    }
                    if (o.cycles != cyc0 || o.energy != 0.0 || o.cap != cap0 || o.prev_power != prev0) s_dirty[h] |= 1;
                    s_cap[h] = o.cap;
                    s_prev[h] = o.prev_power;
                    s_tot[h] = o.tot_e;
                    s_cyc[h] = o.cycles;
                    s_amps[h] = o.energy;
                    if (log_soc) s_abse[h] += fabs(o.energy);
                    stage[0 * RS + h] = o.energy * 60.0 / dtd;
                    stage[(i < nch ? 4 : 5) * RS + h] = fabs(o.energy);
                    stage[6 * RS + h] = (double)o.emerg;
                    stage[7 * RS + h] = o.current;
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        PT_MARK(2)
        lds_barrier();
        }
        PT_MARK(1)

        // ---------------- C: home lanes (from here on everything of one env lives in one wavefront) ----------------
        __builtin_amdgcn_s_waitcnt(0x0F70);   // collect the prefetches before this phase issues stores (vmcnt(0))
        // ... and make that visible to the compiler's wait-count tracking: as outputs of this (empty) asm the
        // prefetched registers are plain values from here on, so their later uses -- after this phase's stores, and
        // across the loop back-edge for the next action -- no longer cost a conservative vmcnt(0) drain
        asm volatile("" : "+v"(a_next), "+v"(pf_pch), "+v"(pf_pdis), "+v"(pf_tr), "+v"(pf_ob0), "+v"(pf_h0), "+v"(pf_h1));
        asm volatile("" : "+v"(pf_c2), "+v"(pf_c7), "+v"(pf_tl), "+v"(pf_d0), "+v"(pf_d1));
        // The fast-forward decision and pass stand HERE, behind the collection point (an EV-free step has no battery-maths phase to run first): a pass
        // that left the step ahead of it gave the loop a second way round on which the compiler had to take the step's prefetches for outstanding, and
        // its vmcnt(0) in front of their registers' first redefinition, at the loop's top, drained the stores of the step before in every step
        // (profiles/r27_step_loop.txt).
        if (FFW && !OUT) asm volatile("" : "+v"(ff_lim_v));   // (read again: nothing of this is kept in a scalar register across phase A)
        const int ff_lim = (FFW && !OUT && EPW == 1) ? __builtin_amdgcn_readfirstlane(ff_lim_v) : 0;
        if (FFW && !OUT && ff_lim != 0) {   // (uniform)
            const uint2 fx = *(const uint2 *)(ffx + 4 * (kk & 1));
            const unsigned f01 = min(fx.x & 0xffffu, fx.x >> 16), f23 = min(fx.y & 0xffffu, fx.y >> 16);
            // EV-free steps from this one on, in all four envs, short of the launch's last step and at most one per lane: the same number in every wavefront
            // (a longer stretch takes another pass, behind the next step's exchange)
            const int n = __builtin_amdgcn_readfirstlane(min(min((int)min(f01, f23), 64), ff_lim - kk));
            if (n >= EV2G_FF_N_MIN) {
                // on to step t + n: its action row (act_run already stands one row behind this step's), requested ahead of the pass and collected with the pass's own loads
                a_next = ldg32_nt<double>(act_run + (long long)(n - 1) * io.a_stride, (unsigned)gc * 8u);
                act_run += (long long)(n - 1) * io.a_stride;
                // all wavefronts have read the four values before any of them writes the next ones: after an even number of steps the parity repeats
                lds_barrier();
                // (sizes and bases from the parameter block, read here: nothing of this rare path is computed ahead of the step loop and kept in scalar registers)
                const int ew = __builtin_amdgcn_readfirstlane(e_l);   // this wavefront's env (lane 0 is its port 0)
                const int Tf = S->T;
                int bx = (int)blockIdx.x;
                asm volatile("" : "+s"(bx));
                // lane i = step t + i.  The pass's loads are issued and collected by EVERY wavefront, one without an env included (its rows are those of the
                // workgroup's first env: valid addresses), so that no way out of the pass leaves a load outstanding
                const int ts = t + lane_l;
                const unsigned row = (unsigned)__builtin_amdgcn_readfirstlane(hb_step) + (unsigned)min(ts, Tf - 1) * 64u;   // the env's scenario's rows in the step table
                d2v tr0 = ldg32_nt<d2v>(S->step_tab, row + 16u), tr1 = ldg32_nt<d2v>(S->step_tab, row + 32u);   // {inflexible + solar, max power}, {min power, setpoint}
                asm volatile("" : "+v"(tr0), "+v"(tr1), "+v"(a_next));
                if (ew < S->E) {
                    double *ea = eacc + (tid_l >> 6) * 7;
                    double n0 = ea[0], n1 = ea[1], n2 = ea[2], n3 = ea[3], n4 = ea[4];
                    const double pot_t = ea[5];   // charge_power_potential of the first step; +0.0 for the later ones
                    // phase E with every per-env sum an exact +0.0
                    const double usage = 0.0, costs = 0.0, user = 0.0;
                    const double tr_power = tr0.x + usage;
                    const double over = (tr_power > tr0.y + 0.0001 || tr_power < tr1.x - 0.0001) ? fabs(tr_power - tr0.y) : 0.0;
                    double reward;
                    if (RK == 1) {
                        const double pp = (lane_l == 0) ? pot_t : 0.0;
                        const double mn = (pp < tr1.y) ? pp : tr1.y;
                        const double d = mn - usage;
                        reward = -(d * d);
                    } else if (RK == 2) {
                        reward = costs - user;
                    } else {
                        reward = costs - 100.0 * over - user;
                    }
                    if (lane_l < n) {   // the step's history row {usage, (potential), overload} and the next row's potential
                        const unsigned h8 = (unsigned)(ew * Tf + ts) * 24u;
                        stg32<double>(S->hist, h8, usage);
                        stg32<double>(S->hist, h8 + 16u, over);
                        if (ts + 1 < Tf) stg32<double>(S->hist, h8 + 32u, 0.0);
                    }
                    // the episode return takes the rewards one by one, in step order, like the steps would
                    const int r_lo = __double2loint(reward), r_hi = __double2hiint(reward);
                    for (int j = 0; j < n; j++)
                        n0 += __hiloint2double(__builtin_amdgcn_readlane(r_hi, j), __builtin_amdgcn_readlane(r_lo, j));
                    n1 += 0.0; n2 += 0.0; n3 += 0.0; n4 += 0.0;   // (x + 0.0 once is x + 0.0 n times)
                    if (lane_l == 0) { ea[0] = n0; ea[1] = n1; ea[2] = n2; ea[3] = n3; ea[4] = n4; ea[5] = 0.0; }
                }
                if (tid_l == 0)
                    __hip_atomic_fetch_add((unsigned long long __attribute__((address_space(1))) *)((gptr)S->ff_count + (unsigned)bx * 8u),
                                           (1ull << 32) | (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                t += n;
                EV2G_STEP_SKIP(n);
            }
        }
        bool occ_any = false;   // an EV on this port before or after the step
        if (FULL && valid && !wave_live && out) {   // the empty wavefront's outputs: zeros
            stg32<uint8_t>(mask, (unsigned)g_l, (uint8_t)0);
            const unsigned ocol_l = (unsigned)((SK == 1) ? 3 + 3 * q_l : (SK == 0 ? 62 + 2 * q_l : 22 + 2 * q_l));
            if (F64) {
                const unsigned o8 = WIDE ? hb_obs_port : hb_obs_env + ocol_l * 8u;
                if (STR_NT) { stg32_nt<d2v>(obs, o8, (d2v){0.0, 0.0}); if (SK == 1) stg32_nt<double>(obs, o8 + 16u, 0.0); }
                else { stg32<d2v>(obs, o8, (d2v){0.0, 0.0}); if (SK == 1) stg32<double>(obs, o8 + 16u, 0.0); }
            }
            if (F32) {
                const unsigned o4 = WIDE ? hb_obs_port : hb_obs_env + ocol_l * 4u;
                if (SK == 1) { stg32<float>(obs32, o4, 0.f); stg32<float>(obs32, o4 + 4u, 0.f); stg32<float>(obs32, o4 + 8u, 0.f); }
                else stg32<f2v>(obs32, o4, (f2v){0.f, 0.f});
                if (ACT) {
                    if (SK == 1 && NWF > 1) { bufXf[arow * FSXF + ocol_l] = 0.f; bufXf[arow * FSXF + ocol_l + 1] = 0.f; bufXf[arow * FSXF + ocol_l + 2] = 0.f; }
                    else
                    if (SK == 1) { bufX[arow * FSX + ocol_l] = 0; bufX[arow * FSX + ocol_l + 1] = 0; bufX[arow * FSX + ocol_l + 2] = 0; }   // (odd columns: three 16-bit words)
                    else xput2((int)ocol_l, 0.f, 0.f);
                }
            }
        }
        if (valid && wave_live) {
            double profit = 0.0, satpen = 0.0, pot = 0.0;
            // every LDS operand of this phase in ONE batch (one wait), whichever branch consumes it: read one by one behind the
            // branches below, each of them was its own LDS round trip on the workgroup-step chain
            int ta = FULL ? r_ta : s_ta[tid_l], td = FULL ? r_td : s_td[tid_l], ss_now = s_ss[tid_l];
            double cap = s_cap[tid_l];
            double b_energy = s_amps[tid_l], b_cur = stage[7 * RS + tid_l], b_ech = stage[4 * RS + tid_l], b_edis = stage[5 * RS + tid_l];
            double b_bcap = FULL ? r_bcap : s_bcap[tid_l], b_potc = FULL ? r_potc : s_potc[tid_l], b_tot = (SK == 1) ? s_tot[tid_l] : 0.0;
            double c_maxp = s_cst[2 * 64 + q_l], c_minp = s_cst[3 * 64 + q_l];
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ta), "+v"(td), "+v"(ss_now), "+v"(cap), "+v"(b_energy), "+v"(b_cur), "+v"(b_ech), "+v"(b_edis),
                         "+v"(b_bcap), "+v"(b_potc), "+v"(b_tot), "+v"(c_maxp), "+v"(c_minp));
            bool departed = false;
            if (occ) {
                const double energy = b_energy;
                const double current = b_cur;
                if (energy != 0.0) {  // profit by the sign of the ACTION (ev_charger.py:178,194), staged under 4 / 5
                    const double ech = b_ech;
                    profit = (ech != 0.0) ? ech * pf_pch : b_edis * pf_pdis;
                }
                if (log_cs && energy != 0.0) {   // charger accumulators (ev_charger.py:178-181,194-197): one lane per charger and step
                    __hip_atomic_fetch_add((double __attribute__((address_space(1))) *)((gptr)S->cs_profits + g8), profit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add((double __attribute__((address_space(1))) *)((gptr)S->cs_e_ch + g8), b_ech, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add((double __attribute__((address_space(1))) *)((gptr)S->cs_e_dis + g8), b_edis, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (current - 0.0001 > c_imax) stg32<int>(S->env_fault, (unsigned)e_l * 4u, 1);  // ev_charger.py:203-205
                if (last_step) { stg32<double>(PA(EV2G_PS_PENERGY), g8, energy); stg32<double>(PA(EV2G_PS_PCURRENT), g8, current); }
                if (log_soc) stg32<double>(S->soc_log + (long long)t * P, g8 + (unsigned)e_l * (unsigned)((T - 1) * P * 8), (current != 0.0) ? cap_before : -cap_before);
                if (t >= td) {  // departure (ev_charger.py:209-229, ev.py:191-214)
                    const int ss = ss_now;
                    const double des = __hiloint2double(pf_tl.y, pf_tl.x);
                    const double score = (cap < des - 0.001) ? cap / des : 1.0;
                    if (RK == 3) satpen = ev2g_departure_term(S->reward_kind, S->cost_kind, score, cap, des);
                    else if (RK != 1 || S->cost_kind == 1) satpen = 100.0 * exp(-10.0 * score);
                    // fire-and-forget device atomics (no returned value => no memory round trip on this path); exactly one
                    // lane updates a given charger per step, so the result does not depend on any ordering
                    __hip_atomic_fetch_add((int __attribute__((address_space(1))) *)(PA(EV2G_PS_SERVED) + (g8 >> 1)), 1,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add((double __attribute__((address_space(1))) *)(PA(EV2G_PS_SATSUM) + g8), score,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    stg32<double>(slabS, (unsigned)ss * 8u, cap);
                    if (log_soc) stg32<double>((slabS + SS8), (unsigned)ss * 8u, s_abse[tid_l]);
                    ta = pf_tl.z; td = pf_tl.w;   // window of the port's next session
                    departed = true;
                    if (FULL) { r_ta = ta; r_td = td; } else { s_ta[tid_l] = ta; s_td[tid_l] = td; }
                    ss_now = (ta != EV2G_INT_MAX) ? ss + 1 : -1;
                    s_ss[tid_l] = ss_now;
                    s_cyc[tid_l] = 0;
                    s_dirty[tid_l] |= 2;
                }
            }
            if (ta == sstep) {  // arrival at the end of this step (ev2gym_env.py:399-417, ev.py:115-136)
                if (departed) {   // the next session arrives right behind a departure of this very step (the reference's spawner leaves a
                                  // gap, replayed scenarios need not): its record was not the one prefetched
                    const unsigned r8 = (unsigned)ss_now * (unsigned)sizeof(SessRec);
                    pf_c2 = ldg32<d2v_a8>(S->rec, r8 + 40u); pf_c7 = ldg32<d2v>(S->rec, r8 + 112u);
                    pf_d0 = ldg32<d2v>(S->sess_dyn, (unsigned)ss_now * 32u); pf_d1 = ldg32<i4v>(S->sess_dyn, (unsigned)ss_now * 32u + 16u);
                }
                cap = pf_c7.x;
                const double B = pf_c2.x;
                const double potc = pf_c7.y;   // v * min(pacmax*1000/v, charger max current) / 1000 (utils.py:773-777), evaluated when the session was loaded
                s_cap[tid_l] = cap; s_tot[tid_l] = 0.0; s_prev[tid_l] = 0.0; s_cyc[tid_l] = 0;
                if (FULL) { r_bcap = B; r_potc = potc; r_rb = pf_c2.y; } else { s_bcap[tid_l] = B; s_potc[tid_l] = potc; }
                s_abse[tid_l] = 0.0;
                b_bcap = B; b_potc = potc; b_tot = 0.0;
                const int lut_new = pf_d1.z;
                stg32<d2v>(wa.lines, l64 + 48u, (d2v){B, potc});   // (the table id travels in s_dirty and reaches the line's head chunk in the epilogue)
                // the attached EV's SessDyn next to its line: what the prologue of a later launch reads (every instantiation writes it)
                stg32<d2v>(wa.port_dyn, (unsigned)g_l * 32u, pf_d0); stg32<i4v>(wa.port_dyn, (unsigned)g_l * 32u + 16u, pf_d1);
                if (FULL) { s_ts[tid_l] = pf_d0.x; s_etac[tid_l] = pf_d0.y; s_etad[tid_l] = __hiloint2double(pf_d1.y, pf_d1.x); }
                stg32<double>(PA(EV2G_PS_PENERGY), g8, 0.0);
                stg32<double>(PA(EV2G_PS_PCURRENT), g8, 0.0);
                s_dirty[tid_l] = (int)((unsigned)((s_dirty[tid_l] & 3) | 1 | ((lut_new + 1) << 8)) | ((FULL && wa.dict) ? (unsigned)pf_d1.w << 20 : 0u));
            }
            const bool occ_after = (ta <= sstep) && (sstep <= td);
            if (RK == 3 && occ_after && S->reward_kind >= 9) {   // (pst_)V2G_profitmaxV2: every connected EV (reward.py:173-195)
                const unsigned r8 = (unsigned)ss_now * (unsigned)sizeof(SessRec);
                satpen += ev2g_connected_term(ldg32<double>(S->tail, (unsigned)ss_now * 16u), cap,
                                              ldg32<double>(S->rec, r8 + (unsigned)offsetof(SessRec, pacmax)), sixty_over_dt, td, sstep);
            }
            occ_any = occ || occ_after;
            if (FULL ? out : mask != nullptr) stg32<uint8_t>(mask, (unsigned)g_l, occ_after ? 1 : 0);
            double o0 = 0.0, o1 = 0.0, o2 = 0.0;
            if (occ_after) {
                const double soc = FULL ? ev2g_fdiv2(cap, b_bcap, r_rb) : cap / b_bcap;   // bit-identical (ev2g_device.h)
                if (SK == 1) { o0 = (soc == 1.0) ? 1.0 : 0.5; o1 = b_tot; o2 = (double)(sstep - ta); }
                else { o0 = soc; o1 = (double)(td - sstep); }
                if (soc < 1.0 && td > sstep) pot = b_potc;  // utils.py:771
            }
            pot = (pot > c_maxp) ? c_maxp : ((pot < c_minp) ? 0.0 : pot);   // per-charger clamp (utils.py:779-789)
            // (the narrow full kernels sit at the register limit: they re-derive the port's column from the env's base)
            const unsigned ocol_l = (unsigned)((SK == 1) ? 3 + 3 * q_l : (SK == 0 ? 62 + 2 * q_l : 22 + 2 * q_l));
            if ((F64 && out) || (!FULL && obs)) {
                const unsigned o8 = WIDE ? hb_obs_port : (FULL ? hb_obs_env + ocol_l * 8u : (unsigned)(e_l * D + ocol) * 8u);
                if (STR_NT) { stg32_nt<d2v>(obs, o8, (d2v){o0, o1}); if (SK == 1) stg32_nt<double>(obs, o8 + 16u, o2); }
                else {
                stg32<d2v>(obs, o8, (d2v){o0, o1});   // one 16-byte store (D and the column offset are even for SK != 1)
                if (SK == 1) stg32<double>(obs, o8 + 16u, o2);
                }
            }
            if ((F32 && out) || (!FULL && obs32)) {
                const unsigned o4 = WIDE ? hb_obs_port : (FULL ? hb_obs_env + ocol_l * 4u : (unsigned)(e_l * D + ocol) * 4u);
                if (SK == 1) { stg32<float>(obs32, o4, (float)o0); stg32<float>(obs32, o4 + 4u, (float)o1); stg32<float>(obs32, o4 + 8u, (float)o2); }
                else stg32<f2v>(obs32, o4, (f2v){(float)o0, (float)o1});
                if (ACT) {   // the policy's copy of the same columns
                    if (SK == 1 && NWF > 1) { bufXf[arow * FSXF + ocol_l] = (float)o0; bufXf[arow * FSXF + ocol_l + 1] = (float)o1; bufXf[arow * FSXF + ocol_l + 2] = (float)o2; }
                    else
                    if (SK == 1) {
                        const uint32_t w01 = ev2g_pack_bf16((float)o0, (float)o1), w2 = ev2g_pack_bf16((float)o2, 0.f);
                        bufX[arow * FSX + ocol_l] = (uint16_t)w01; bufX[arow * FSX + ocol_l + 1] = (uint16_t)(w01 >> 16); bufX[arow * FSX + ocol_l + 2] = (uint16_t)w2;
                    } else xput2((int)ocol_l, (float)o0, (float)o1);
                }
            }
            if (log_cs) {   // cs_power / cs_current of the step (ev2gym_env.py:533-535) and the chargers' current_power_output / current_total_amps
                const double pw = occ ? stage[0 * RS + tid_l] : 0.0, cur = occ ? b_cur : 0.0;
                const unsigned hc8 = ((unsigned)(t * E + e_l) * (unsigned)P + (unsigned)q_l) * 8u;
                stg32<double>(S->cs_power_hist, hc8, pw); stg32<double>(S->cs_cur_hist, hc8, cur);
                if (last_step) { stg32<double>(S->cs_power_now, g8, pw); stg32<double>(S->cs_cur_now, g8, cur); }
            }
            stage[1 * RS + tid_l] = profit;
            stage[2 * RS + tid_l] = satpen;
            stage[3 * RS + tid_l] = pot;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wavefront's LDS writes are visible to itself
        PT_MARK(3)

        // ---------------- D: per-env reduction inside the wavefront (fixed tree: bit-reproducible) ----------------
        // lane = k*8 + j: quantity k, chain j.  Every lane issues its 8 LDS reads unconditionally (clamped index, masked
        // by a select; the slots of idle lanes hold zeros), sums two chains, and three DPP xor-butterflies leave env w's
        // sum of quantity k in lane k*8.  That lane parks it in the env's head slot of the stage row it just reduced
        // (stage[k][first port of env w]; only this lane ever reads that slot in this phase), where the head lane --
        // the only consumer of env-level sums -- picks all eight up below.  LDS operations of one wavefront execute in
        // order, so no barrier is involved.
        // A wavefront whose envs hold no EV before or after this step (the night half of a workplace episode, the early
        // morning) has nothing to add up: every staged value of its ports is an exact +0.0.
        double esum[EV2G_NQ];
#pragma unroll
        for (int kq = 0; kq < EV2G_NQ; kq++) esum[kq] = 0.0;
        // SquaredTrackingErrorRewardWithPenalty only (a run-time reward): the port powers once more, charger by charger like the reference
        // (RewardIn::usage_seq, ev2g_device.h) -- by the env's head lane, before the reduction parks the env's sum in its first slot
        double useq = 0.0;
        if (RK == 3 && S->reward_kind == 4 && head) {
            const double *prow = stage + tid_l;   // slot == reference port on this path (one transformer, single-port chargers)
            for (int c0 = 0; c0 < P; c0 += 8) {
                double x[8];
#pragma unroll
                for (int i = 0; i < 8; i++) x[i] = prow[min(c0 + i, P - 1)];
#pragma unroll
                for (int i = 0; i < 8; i++) if (c0 + i < P) useq += x[i];
            }
        }
        if (__ballot(occ_any) != 0ull) {   // (uniform)
        {
            const int k = lane_l >> 3, j = lane_l & 7;
            const int wbase = (tid_l & ~63);
            const double *row = stage + k * RS;
            // The order of the additions is the same in every branch (chains j, j+16, j+32, j+48 and j+8, j+24, j+40, j+56, then the
            // butterfly); the branches differ in which of the operands they know to be zero without looking.
            if (EPW == 1) {   // (uniform) one env per wavefront: the slots behind its last port belong to idle lanes and still hold the
                              // zeros they were initialised with -- eight reads at constant offsets, no masks, no index clamps
                const double *r0 = row + wbase + j;
                double xa[4], xb[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { xa[u] = r0[16 * u]; xb[u] = r0[16 * u + 8]; }
                double acc = 0.0, accb = 0.0;
#pragma unroll
                for (int u = 0; u < 4; u++) { acc += xa[u]; accb += xb[u]; }
                acc += accb;
                acc += xor1_f64(acc);
                acc += xor2_f64(acc);
                acc += xor4_f64(acc);
                // lane 8k now holds the env's sum of quantity k: with ONE env per wavefront the sums are wave-uniform, so they are
                // read out with v_readlane (scalar registers) instead of being parked in LDS and read back by every lane --
                // two LDS round trips less on the step's chain.  (Quantity 7, the summed current, has no consumer on this path.)
                const int acc_lo = __double2loint(acc), acc_hi = __double2hiint(acc);
#pragma unroll
                for (int kq = 0; kq < EV2G_NQ - 1; kq++)
                    esum[kq] = __hiloint2double(__builtin_amdgcn_readlane(acc_hi, kq * 8), __builtin_amdgcn_readlane(acc_lo, kq * 8));
            } else {          // several envs per wavefront: P <= 32, so ports j+32 .. j+56 do not exist (their terms were exact zeros);
                              // an unclamped index past the env reads a neighbour's slot (or, behind the last row, the array that
                              // follows `stage` in LDS) and is masked
                const bool upper = P > 16;   // (uniform)
                // two or three envs per wavefront (the PublicPST benchmark shape: 3 x 20 ports): their reductions are independent -- all LDS
                // reads first, then the three add / butterfly chains side by side -- instead of one env after the other, each behind its own
                // LDS round trip (1.9 k of a workgroup-step's 10.8 k ticks at cfg3)
                auto envs_at_once = [&](auto NEc) __attribute__((always_inline)) {
                    constexpr int NE = decltype(NEc)::value;
                    double ra0[NE], rb0[NE], ra1[NE], rb1[NE];
#pragma unroll
                    for (int w = 0; w < NE; w++) {
                        const double *r0 = row + wbase + w * ES + j;
                        ra0[w] = r0[0]; rb0[w] = r0[8]; ra1[w] = 0.0; rb1[w] = 0.0;
                        if (upper) { ra1[w] = r0[16]; rb1[w] = r0[24]; }
                    }
                    double acc[NE];
#pragma unroll
                    for (int w = 0; w < NE; w++) {
                        const int a = wbase + w * ES, b = a + P, i = a + j;
                        double ac = 0.0, accb = 0.0;
                        ac += (i < b) ? ra0[w] : 0.0;
                        accb += (i + 8 < b) ? rb0[w] : 0.0;
                        if (upper) { ac += (i + 16 < b) ? ra1[w] : 0.0; accb += (i + 24 < b) ? rb1[w] : 0.0; }
                        acc[w] = ac + accb;
                    }
#pragma unroll
                    for (int w = 0; w < NE; w++) acc[w] += xor1_f64(acc[w]);
#pragma unroll
                    for (int w = 0; w < NE; w++) acc[w] += xor2_f64(acc[w]);
#pragma unroll
                    for (int w = 0; w < NE; w++) acc[w] += xor4_f64(acc[w]);
#pragma unroll
                    for (int w = 0; w < NE; w++) if (j == 0) stage[k * RS + wbase + w * ES] = acc[w];
                };
                if (EPW == 3) envs_at_once(std::integral_constant<int, 3>{});
                else if (EPW == 2) envs_at_once(std::integral_constant<int, 2>{});
                else
#pragma unroll 1
                for (int w = 0; w < EPW; w++) {
                    const int a = wbase + w * ES, b = a + P;
                    const double *r0 = row + a + j;
                    const double ra0 = r0[0], rb0 = r0[8];
                    double ra1 = 0.0, rb1 = 0.0;
                    if (upper) { ra1 = r0[16]; rb1 = r0[24]; }
                    const int i = a + j;
                    double acc = 0.0, accb = 0.0;
                    acc += (i < b) ? ra0 : 0.0;
                    accb += (i + 8 < b) ? rb0 : 0.0;
                    if (upper) { acc += (i + 16 < b) ? ra1 : 0.0; accb += (i + 24 < b) ? rb1 : 0.0; }
                    acc += accb;
                    acc += xor1_f64(acc);
                    acc += xor2_f64(acc);
                    acc += xor4_f64(acc);
                    if (j == 0) stage[k * RS + a] = acc;
                }
            }
        }
        if (EPW != 1) {   // (uniform)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int kq = 0; kq < EV2G_NQ - 1; kq++) esum[kq] = stage[kq * RS + (tid_l - q_l)];   // the env's sums (its head slot), every lane (quantity 7, the summed current, has no consumer on this path)
        }
        }

        PT_MARK(4)
        // ---------------- E: per env (head lane) + observation head (the env's lanes) ----------------
        const double usage = esum[0];
        // {min_power, setpoint} from the next lane (wave_shl:1 -- the head lane's neighbour always belongs to the same env)
        const double pf_base = pf_tr.x, pf_maxp = pf_tr.y;
        const double pf_minp = dpp_mov_f64<0x130>(pf_tr.x), pf_sp = dpp_mov_f64<0x130>(pf_tr.y);
        // Transformer.reset + step + get_how_overloaded (transformer.py:258-302), evaluated wave-wide (meaningful in head lanes)
        const double tr_power = pf_base + usage;   // inflexible_load[t] + solar_power[t] + sum of the charger powers
        const double over = (tr_power > pf_maxp + 0.0001 || tr_power < pf_minp - 0.0001) ? fabs(tr_power - pf_maxp) : 0.0;
        if (WIDE || P >= 3) {
            // the three history entries of the step in ONE store: lane 0 of the env writes usage[t], lane 1 the overload
            // (handed over by a DPP wave shift), lane 2 potential[t+1] -- not three stores with one active lane each
            const double over_n = dpp_mov_f64<0x138>(over);   // wave_shr:1: lane L takes lane L-1's value
            if (valid && q_l < 3 && (q_l != 2 || sstep < T)) {
                const double hv = (q_l == 0) ? usage : ((q_l == 1) ? over_n : esum[3]);
                // row (e, t) of the history array [E, T, 3]: words {usage, potential, overload}; lane 2 writes into row t + 1 -- 40 bytes in all
                const unsigned hword = (q_l == 0) ? 0u : ((q_l == 1) ? 16u : 32u);
                stg32<double>(hist + (long long)t * 24, (unsigned)(e_l * T) * 24u + hword, hv);
            }
        }
        if (head) {
            double *ea = eacc + elg * 7;
            // all six accumulator words are read up front (one LDS wait) and written back together at the end; reading
            // each one next to its update made every update wait for its own LDS round trip
            const double ea0 = ea[0], ea1 = ea[1], ea2 = ea[2], ea3 = ea[3], ea4 = ea[4], ea5 = ea[5];
            const double ea6 = (RK == 3) ? ea[6] : 0.0;
            const unsigned e8 = (unsigned)e_l * 8u;
            double over100 = 0.0;
            if (RK == 0 || RK == 3) over100 = 100.0 * over;
            if (last_step) stg32<double>(S->tr_power_now, e8, tr_power);
            const double potn = esum[3];
            if (!WIDE && P < 3) {   // two-port envs: no third lane to share the history stores with
                const unsigned h8 = (unsigned)(e_l * T + t) * 24u;
                stg32<double>(hist, h8 + 16u, over);
                stg32<double>(hist, h8, usage);
                if (sstep < T) stg32<double>(hist, h8 + 32u, potn);
            }
            const double costs = esum[1];
            double reward;
            if (RK == 1) {  // SquaredTrackingErrorReward reward.py:7-14
                const double pp = ea5;
                const double m = (pp < pf_sp) ? pp : pf_sp;
                const double d = m - usage;
                reward = -(d * d);
            } else if (RK == 2) {  // profit_maximization reward.py:78-87
                reward = costs - esum[2];
            } else if (RK == 3) {  // the other fused rewards, by V2P::reward_kind
                RewardIn ri;
                ri.costs = costs; ri.usage = usage; ri.usage_seq = (S->reward_kind == 4) ? useq : usage; ri.sp = pf_sp; ri.pot_t = ea5; ri.pot_tm1 = ea6; ri.over100 = over100;
                ri.user = esum[2]; ri.tr0_maxp = pf_maxp;
                reward = ev2g_reward(S->reward_kind, ri);
            } else {  // ProfitMax_TrPenalty_UserIncentives reward.py:34-44
                reward = costs - over100 - esum[2];
            }
            const double n0 = ea0 + reward, n1 = ea1 + costs, n2 = ea2 + esum[4], n3 = ea3 + esum[5], n4 = ea4 + esum[6];
            ea[0] = n0; ea[1] = n1; ea[2] = n2; ea[3] = n3; ea[4] = n4; ea[5] = potn;
            if (RK == 3) ea[6] = ea5;
            if (FULL && out) { stg32<double>(rew_run, e8, reward); stg32<uint8_t>(done_run, (unsigned)e_l, (sstep >= T) ? 1 : 0); }
            if (!FULL && io.reward) stg32<double>(io.reward + (long long)kk * io.r_stride, e8, reward);
            if (!FULL && io.done) stg32<uint8_t>(io.done + (long long)kk * io.d_stride, (unsigned)e_l, (sstep >= T) ? 1 : 0);
            if (!FULL && S->x_cost)   // cost_function (rl_agent/cost.py:8-27); the overload weight is applied here when the reward does not carry it
                stg32<double>(S->x_cost + (long long)(io.step0 + kk) * S->x_c_stride, e8, (S->cost_kind == 2) ? costs : 100.0 * over + esum[2]);
            if (sstep >= T || last_step) {  // publish the running episode totals (get_statistics reads them)
                const unsigned a8 = (unsigned)e_l * 64u;
                if (FFW) {   // (the base from the parameter block, here: a launch publishes once, and the pointer is not held in scalar registers across the step loop)
                    stg32<d2v>(S->env_acc, a8, (d2v){n0, n1});
                    stg32<d2v>(S->env_acc, a8 + 16u, (d2v){n2, n3});
                    stg32<double>(S->env_acc, a8 + 32u, n4);
                } else {
                    stg32<d2v>(env_acc, a8, (d2v){n0, n1});
                    stg32<d2v>(env_acc, a8 + 16u, (d2v){n2, n3});
                    stg32<double>(env_acc, a8 + 32u, n4);
                }
            }
        }
        if ((valid || hcopy) && ((F32 && out) || (!FULL && obs32))) {
            const unsigned o4 = FULL ? hb_obs_env : (unsigned)(e_l * D) * 4u;
            if (SK == 1) {
                if (q_l == 0) {
                    const float h0 = (float)((double)sstep / (double)T), h1 = (float)((sstep < T) ? pf_ob0 : 0.0), h2 = (float)usage;
                    stg32<float>(obs32, o4, h0);
                    stg32<float>(obs32, o4 + 4u, h1);
                    stg32<float>(obs32, o4 + 8u, h2);
                    if (ACT && NWF > 1) { bufXf[arow * FSXF] = h0; bufXf[arow * FSXF + 1] = h1; bufXf[arow * FSXF + 2] = h2; }
                    else
                    if (ACT) {   // the policy's copy: columns 0, 1 as one word, column 2 on its own (column 3 belongs to port 0)
                        *(uint32_t *)(bufX + arow * FSX) = ev2g_pack_bf16(h0, h1);
                        bufX[arow * FSX + 2] = (uint16_t)ev2g_pack_bf16(h2, 0.f);
                    }
                }
            } else {
                if (q_l == 0) stg32<f2v>(obs32, o4, (f2v){(float)sstep, (float)usage});
                if (q_l < NPAIR) stg32<f2v>(obs32, o4 + 8u + (unsigned)q_l * 8u, (f2v){(float)pf_h0.x, (float)pf_h0.y});
                if (ACT) {
                    if (q_l == 0) xput2(0, (float)sstep, (float)usage);
                    if (q_l < NPAIR) xput2(2 + 2 * q_l, (float)pf_h0.x, (float)pf_h0.y);
                }
                if (!WIDE) {
                    if (q_l + P < NPAIR) stg32<f2v>(obs32, o4 + 8u + (unsigned)(q_l + P) * 8u, (f2v){(float)pf_h1.x, (float)pf_h1.y});
                    const unsigned h8 = (unsigned)((scn * (T + 1) + sstep) * NHEAD) * 8u;
                    for (int pi = q_l + 2 * P; pi < NPAIR; pi += P) {
                        const d2v hv = ldg32<d2v>(S->head_tab, h8 + (unsigned)pi * 16u);
                        stg32<f2v>(obs32, o4 + 8u + (unsigned)pi * 8u, (f2v){(float)hv.x, (float)hv.y});
                    }
                }
            }
        }
        if (valid && ((F64 && out) || (!FULL && obs))) {
            const unsigned o8 = FULL ? hb_obs_env : (unsigned)(e_l * D) * 8u;
            if (SK == 1) {  // PublicPST state.py:6-35
                if (q_l == 0) {
                    stg32<double>(obs, o8, (double)sstep / (double)T);
                    stg32<double>(obs, o8 + 8u, (sstep < T) ? pf_ob0 : 0.0);
                    stg32<double>(obs, o8 + 16u, usage);
                }
            } else {  // V2G_profit_max(_loads) state.py:65-83, :108-135: columns 2.. are a copy of the head table row
                if (STR_NT) {
                    if (q_l == 0) stg32_nt<d2v>(obs, o8, (d2v){(double)sstep, usage});
                    if (q_l < NPAIR) stg32_nt<d2v>(obs, o8 + 16u + (unsigned)q_l * 16u, pf_h0);
                } else {
                if (q_l == 0) stg32<d2v>(obs, o8, (d2v){(double)sstep, usage});
                if (q_l < NPAIR) stg32<d2v>(obs, o8 + 16u + (unsigned)q_l * 16u, pf_h0);
                }
                if (!WIDE) {
                    if (q_l + P < NPAIR) stg32<d2v>(obs, o8 + 16u + (unsigned)(q_l + P) * 16u, pf_h1);
                    const unsigned h8 = (unsigned)((scn * (T + 1) + sstep) * NHEAD) * 8u;
                    for (int pi = q_l + 2 * P; pi < NPAIR; pi += P)    // tiny envs (P < 15): the remaining pairs, unprefetched
                        stg32<d2v>(obs, o8 + 16u + (unsigned)pi * 16u, ldg32<d2v>(S->head_tab, h8 + (unsigned)pi * 16u));
                }
            }
        }
        PT_MARK(5)
        PT_STEP_END(cntk[0] + cntk[1] == 0)
        t += 1;
        if (STR) { obs_run += io.o_stride; rew_run += io.r_stride; done_run += io.d_stride; mask_run += io.m_stride; }
        if (ACT) obs32_run += io.o_stride;
        // The next step's phase A rewrites stage[0,4..7] / s_amps of this wavefront's own lanes only after this
        // wavefront finished reading them (program order); other wavefronts never touch these slots outside phase B,
        // which is fenced by the two barriers.
