// ev2g_step_wave.h -- fast path of the step kernel for the common shape: P <= 64 ports per env, one transformer,
// single-port chargers (BASELINE cfg2 / cfg3 / cfg5 and the reference's shipped YAML files).
//
// Same phases and the same arithmetic as ev2g_step_v2 (ev2g_step_v2.h), with two structural differences:
//   * WAVE-ALIGNED envs: a wavefront owns EPW = 64 / P whole envs (lanes [0, EPW*P)).  Everything that concerns one
//     env after the battery maths -- departures / arrivals, observation columns, the per-env reduction, transformer
//     overload, reward, observation head -- then happens inside ONE wavefront, ordered by s_waitcnt only.  Only the
//     compaction hand-off (home lanes -> worker lanes -> home lanes) crosses wavefronts, so a step has TWO workgroup
//     barriers instead of five or six.
//   * specialised at compile time on the fused (state, reward) plugin pair, so the plugin branches, their loads and
//     their registers disappear.
// The reduction is still LDS-staged and fixed-order (8 quantities x 8 lanes, two chains, 3 xor steps), i.e.
// bit-reproducible, and identical in value to the generic kernel's (same tree).
#pragma once
#include <type_traits>
#include "ev2g_step_v2.h"
#include "ev2g_mlp.h"
#include "ev2g_timing_host.h"

#define EV2G_WAVE_BLOCK 256
// the shortest EV-free stretch ev2g_step_wave fast-forwards (FFW): a one-step pass costs a barrier and one memory round trip, like the step it replaces
#ifndef EV2G_FF_N_MIN
#define EV2G_FF_N_MIN 1
#endif

__host__ __device__ inline size_t ev2g_wave_lds_bytes(int envs_per_group, int block = EV2G_WAVE_BLOCK) {
    const size_t NS = (size_t)block;
    return sizeof(double) * (EV2G_NQ * (NS + 8) + 7 * NS + 7 * (size_t)envs_per_group + 4 * 64) + sizeof(int) * (6 * NS + 8);
}
// the in-launch statistics phase (end of ev2g_step_wave): SoC-log entries per session kept in registers / parked in LDS (a multiple of
// EV2G_STATS_TB; the whole workgroup's blocks, BLOCK / 64 x LK x 64 doubles, must fit the step's LDS -- checked by the host)
#define EV2G_INL_STATS_NK 12
#define EV2G_INL_STATS_LK 16
__host__ __device__ inline size_t ev2g_inl_stats_lds_bytes(int block = EV2G_WAVE_BLOCK) { return (size_t)block * EV2G_INL_STATS_LK * sizeof(double); }
// the fused actor + step instantiation (ACT, below): 16 envs and 16 wavefronts per workgroup, plus the policy's input rows (bf16) and its actions (float) in LDS
#define EV2G_FUSED_BLOCK 1024
#define EV2G_FUSED_SX 200     // MlpS16<6, ..>::SX: bf16 elements per observation row in LDS
#define EV2G_FUSED_RING 10    // weight fragments a wavefront keeps in flight (ev2g_mlp3_inline)
#define EV2G_FUSED_RING2 7    // the same with two envs per wavefront (AE = 2): the second row block's accumulators and operand take 12 registers

#define EV2G_FUSED_SXF 196    // the float32 policy (NWF = 2): floats per observation row in LDS (6 k-steps of 32 + 16 bytes against bank conflicts)
#define EV2G_FUSED_RINGF 4    // ... and its weight fragments in flight per wavefront (two terms per k-step; 6 / 8 measure the same as 4 and leave no registers for reading the next k-step's operands ahead)
__host__ __device__ inline size_t ev2g_fused_lds_bytes(int envs_per_wave = 1, int weight_terms = 1) {
    if (weight_terms > 1)   // float32 input rows (H2's third copy lies over them between layers 1 and 3), biases from global memory: 163 488 of the 163 840 bytes
        return ev2g_wave_lds_bytes(EV2G_FUSED_BLOCK / 64 * envs_per_wave, EV2G_FUSED_BLOCK) + (size_t)16 * EV2G_FUSED_SXF * 4;
    return ev2g_wave_lds_bytes(EV2G_FUSED_BLOCK / 64 * envs_per_wave, EV2G_FUSED_BLOCK) + (size_t)16 * EV2G_FUSED_SX * 2 + (size_t)(25 + 19 + 4) * 16 * 4;   // + input rows, biases
}
// What the fused instantiation needs besides the step's own arguments: the policy, and the observation rows its first forward reads.
// StepIO then carries the OUTPUT blocks: obs32 = the rows the steps write (row of the launch's first step; o_stride floats between steps, 0: one row
// overwritten, and then obs0 == obs32), act32 = the action rows the policy writes (a_stride floats between steps), reward / done / mask with their strides.
struct FusedArgs {
    MlpDev m;
    const float *obs0;
};

// Global accesses as  uniform base (an SGPR pair) + 32-bit unsigned BYTE offset (one VGPR):  the
// `global_load/store v, v_off, s[base:base+1]` form.  Indexing a pointer with a (sign-extended) int instead makes every
// access carry a 64-bit VALU address computation (v_ashrrev + v_lshl_add_u64, an address VGPR pair each).  The host
// selects this kernel only when every array it addresses is smaller than 4 GiB (ev2g_host.hip).
typedef const char __attribute__((address_space(1))) *gcptr;
typedef char __attribute__((address_space(1))) *gptr;
template <class T, class B> __device__ __forceinline__ T ldg32(B base, unsigned boff) {
    return *(const T __attribute__((address_space(1))) *)((gcptr)base + boff);
}
// streaming variant: read once per step and never again by this CU -- keep it from displacing the session records and
// efficiency tables (re-read every step) in the vector L1
template <class T, class B> __device__ __forceinline__ T ldg32_nt(B base, unsigned boff) {
    return __builtin_nontemporal_load((const T __attribute__((address_space(1))) *)((gcptr)base + boff));
}
template <class T, class B> __device__ __forceinline__ void stg32(B base, unsigned boff, T v) {
    *(T __attribute__((address_space(1))) *)((gptr)base + boff) = v;
}
template <class T, class B> __device__ __forceinline__ void stg32_nt(B base, unsigned boff, T v) {   // streaming store: written once, read by another kernel if at all
    __builtin_nontemporal_store(v, (T __attribute__((address_space(1))) *)((gptr)base + boff));
}
typedef double d2v __attribute__((ext_vector_type(2)));   // builtin vectors: loadable from any address space
typedef double d2v_a8 __attribute__((ext_vector_type(2), aligned(8)));   // the same at an 8-byte aligned address (global_load_dwordx4 needs dword alignment only)
typedef int i2v __attribute__((ext_vector_type(2)));
typedef int i4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
// The battery-maths part of the record in one memory round trip: the chunks this wavefront's kind of step reads (charging 0..4, discharging
// 3..6; uniform -- the two lists start on wavefront boundaries), issued back to back, then pinned by an empty asm so that the compiler cannot
// sink the ones a later branch does not need behind that branch (it otherwise loads the gate field first and the rest only after testing
// it: two dependent round trips).
template <class B> __device__ __forceinline__ SessRec ldg32_rec_charge(B base, unsigned boff) {
    union { SessRec r; d2v v[sizeof(SessRec) / 16]; } u;
    static_assert(sizeof(SessRec) == 128 && offsetof(SessRec, rB) == 48 && offsetof(SessRec, rv) == 64 && offsetof(SessRec, minB) == 80 && offsetof(SessRec, cap0) == 112,
                  "charging reads chunks 0..4, discharging chunks 3..6");
#pragma unroll
    for (int i = 0; i < 5; i++) u.v[i] = ldg32<d2v>(base, boff + 16u * i);
    asm volatile("" : "+v"(u.v[0]), "+v"(u.v[1]), "+v"(u.v[2]), "+v"(u.v[3]), "+v"(u.v[4]));
    return u.r;
}
template <class B> __device__ __forceinline__ SessRec ldg32_rec_discharge(B base, unsigned boff) {
    union { SessRec r; d2v v[sizeof(SessRec) / 16]; } u;
#pragma unroll
    for (int i = 3; i < 7; i++) u.v[i] = ldg32<d2v>(base, boff + 16u * i);
    asm volatile("" : "+v"(u.v[3]), "+v"(u.v[4]), "+v"(u.v[5]), "+v"(u.v[6]));
    return u.r;
}

// Round 5 (full kernels): the same operands from the dictionary entry (ClsRec, ev2g_device.h) -- four chunks for a charging step, three for a
// discharging one -- with the per-session ones (transition_soc, the efficiencies) supplied by the caller from the port's LDS state.
template <class B> __device__ __forceinline__ SessRec ldg32_cls_charge(B base, unsigned boff) {
    static_assert(sizeof(ClsRec) == 128 && offsetof(ClsRec, gate_ch) == 16 && offsetof(ClsRec, rB) == 32 && offsetof(ClsRec, rv) == 48 && offsetof(ClsRec, v_d) == 64 &&
                  offsetof(ClsRec, gate_dis) == 80 && offsetof(ClsRec, emerg) == 96, "ClsRec layout");
    d2v c[4];
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = ldg32<d2v>(base, boff + 16u * i);
    asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
    SessRec r;
    r.pacmax = c[0].x; r.tsm = c[0].y; r.gate_ch = c[1].x; r.B = c[1].y; r.rB = c[2].x; r.v = c[2].y; r.rv = c[3].x;
    return r;
}
template <class B> __device__ __forceinline__ SessRec ldg32_cls_discharge(B base, unsigned boff) {
    d2v c[3];
#pragma unroll
    for (int i = 0; i < 3; i++) c[i] = ldg32<d2v>(base, boff + 64u + 16u * i);
    asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]));
    SessRec r;
    r.v = c[0].x; r.rv = c[0].y; r.gate_dis = c[1].x; r.minB = c[1].y; r.emerg = c[2].x; r.pdismax = c[2].y;
    return r;
}

// What the launch prologue needs, BY VALUE: with it the first data loads depend on one fetch (the kernarg segment)
// instead of two (kernarg -> parameter block).  A launch starts with cold caches, so every dependent fetch in the
// prologue is a full memory round trip -- paid per step by single-step launches.
struct WaveArgs {
    int P, T, E, D, M;
    char *slab_port; unsigned long long slab_port_slice;
    double *hist;            // [E, T, 3] usage | potential | overload per (env, step) (one transformer)
    double *env_acc;
    const double *cs_pack;   // [C][6] imax, |dmax|, imin, dmin, max power, min power
    char *lines;             // [E*P] PortLine
    const double *step_tab;  // [M, T, 8]; slots 6, 7: the scenario's occupancy / arrival masks of the step
    char *port_dyn;          // [E*P] PortDyn: transition_soc, efficiencies, table id and dictionary entry of the attached EV
    int dict;                // DevScn::dict: V2P::cls_rec is a dictionary (entry = bits 20..31 of the port's LDS word); 0: one ClsRec per session
    int epw, es;             // envs per wavefront (<= 64 / P) and the lane stride between them (>= P; P: packed, 64 / epw: aligned to lane rows)
    const int *grp_map = nullptr;   // [gridDim.x] the env group of every workgroup (a permutation, ev2g_balance_host.h); nullptr: the kernel's own map
    // launch stamps (ev2g_timing_host.h): two words of the handle's ring -- [0] the constant-rate wall clock in workgroup 0's prologue, [1] the largest
    // one a workgroup read at its exit (behind a barrier: one atomic maximum per workgroup); nullptr: the launch is timed by events around it, or not at all, and the kernel does what it always did
    unsigned long long *stamp = nullptr;
};
// The kernel-argument segment of ev2g_step_wave as a struct: where the two stamp sites fetch WaveArgs::stamp from, each for itself -- taken from `wa` the
// pointer would be a scalar register pair held (or parked in lanes) across the whole step loop, like the output pointers before the peeled step.
// It MUST follow the kernel's parameter list up to and including `wa` (the trailing FusedArgs is left out): a parameter inserted in front of `wa`
// without its twin here would make the sites read another word as the pointer.
struct WaveKernArgs {
    const void *params; StepIO io; int t0, k_steps, auto_reset; WaveArgs wa;
};
static_assert(offsetof(WaveKernArgs, io) == 8 && offsetof(WaveKernArgs, t0) == 8 + sizeof(StepIO) && alignof(WaveArgs) == 8 &&
              offsetof(WaveKernArgs, wa) == ((8 + sizeof(StepIO) + 3 * sizeof(int) + 7) & ~(size_t)7),
              "WaveKernArgs lays the parameters out the way the kernel-argument segment does: each at its natural alignment, in order");
__device__ __forceinline__ unsigned long long *ev2g_wave_stamp_arg() {
    const char __attribute__((address_space(4))) *kargs = (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kargs));
    return *(unsigned long long *const __attribute__((address_space(4))) *)(kargs + offsetof(WaveKernArgs, wa) + offsetof(WaveArgs, stamp));
}

// IO32: the actions are float32 (StepIO::act32) -- the policy-network interface; float32 observations (StepIO::obs32) are
// written whenever that pointer is set, in either instantiation.
// RK: 0..2 = the reward of the three shipped configs, compiled in; 3 = any other fused reward, selected at run time by
// V2P::reward_kind (ev2g_reward / ev2g_departure_term in ev2g_device.h).
// FULL (with IO32: the same for the policy network's hand-over -- float32 actions in, the float32 observation out INSTEAD of the float64
// one; what ev2g_rollout launches between two actor forwards):
// the launch writes all four float64 outputs (observation, reward, done, mask) with step stride 0 (one buffer that holds the launch's
// last step: what a loop that consumes them step by step, or a benchmark, passes -- only the LAST step of a longer launch writes them,
// LSO below: the earlier rows could never be seen), takes float64 actions, uses no extras (fused cost, float32
// observations, charger histories) and contains no in-launch reset.  The null checks, the extras' parameter fetches, the outputs'
// per-step pointer arithmetic and the reset branch -- dozens of scalar instructions a step, issued by every wavefront -- are compiled
// out: measured 4.53 -> 4.28 us/step at cfg2, 5.40 -> 5.08 at cfg3 (the kernel's time is its instruction count, SURVEY par.8d / DESIGN par.3).
// FULLK = 2 additionally knows at compile time that the SoC log is on (EV2G_FLAG_LOG_SOC: the Python surface's and the benchmark's default)
// and that the env is wide enough for one observation-head column pair per lane (P >= 30 for the 60-column head, P >= 10 for the
// 20-column one): the second pair's prefetch and stores and the tail loop of narrow envs go too.
// FULLK = 3 (round 5) is FULLK = 2 for outputs with STEP STRIDES -- the [K, E, *] blocks of a persistent launch whose every observation, reward, done
// flag and mask is kept (generate_trajectories.py:69-83 style use; a replay block): four running pointers advanced with scalar adds per step,
// everything else as compiled-out as in 2.
// ACT (round 5; BLOCK = 1024, FULLK = 2, IO32): the policy network (FusedArgs::m, obs -> 400 -> 300 -> ports on the bf16 matrix cores) is evaluated INSIDE
// the launch, between the steps, by the workgroup that steps the 16 envs whose rows it reads: one launch per rollout segment of k steps (ev2g_collect /
// ev2g_rollout) instead of two per step -- no kernel boundary, so no cold start of either kernel, the port state stays in LDS across the segment
// like in any persistent launch, observations reach the policy and actions reach the step through LDS, and the weights are streamed once per CU and step.
// The outputs (observation / action / reward / done / mask rows of every step) go to the caller's blocks through running pointers.
// AE (round 6; ACT with PublicPST, P <= 32): TWO envs per wavefront in the fused instantiation (lanes 0..31 / 32..63), 32 policy rows per workgroup -- every weight
// fragment feeds two MFMAs, the weight stream per env halves, and 8192 envs are one round of 256 workgroups instead of two rounds of 512.
// NWF (round 6, last session; ACT with a head-table state, AE = 1): the FLOAT32 policy (EV2G_MLP_F32: two bf16 terms per weight, three per activation)
// inside the launch -- ev2g_mlp3_inline_f32 (ev2g_mlp.h): the input rows stay float32 in LDS, the hidden activations' three copies fill the staging rows.
// (the parameter list is mirrored by WaveKernArgs above, which the launch-stamp sites read `wa.stamp` through: change the two together)
template <int SK, int RK, bool IO32, int FULLK = 0, int BLOCK = EV2G_WAVE_BLOCK, bool ACT = false, int AE = 1, int NWF = 1>
__global__ void __launch_bounds__(BLOCK, 4) ev2g_step_wave(const V2P *__restrict__ params, StepIO io, int t0,
                                                           int k_steps, int auto_reset, WaveArgs wa, FusedArgs fa) {
    extern __shared__ double lds[];
    static_assert(!ACT || (IO32 && FULLK == 2 && BLOCK == EV2G_FUSED_BLOCK), "the fused actor + step instantiation");
    static_assert(AE == 1 || (ACT && SK == 1 && AE == 2), "two envs per wavefront in the fused instantiation: PublicPST only");
    static_assert(NWF == 1 || (ACT && AE == 1 && NWF == 2), "the float32 policy inside the launch: one env per wavefront (16 policy rows per workgroup)");
    constexpr bool FULL = FULLK >= 1, WIDE = FULLK >= 2, STR = FULLK >= 3 || ACT;
    constexpr bool STR_NT = FULLK >= 3;   // the kept observation rows (0.6 GB per cfg2 launch) as streaming stores: they should not displace the state lines in L2 (-2 %, profiles/r05_ab_strided_nt.txt)
    constexpr bool F64 = FULL && !IO32, F32 = FULL && IO32;   // full with float64 actions in / observations out, or with the float32 hand-over
    // LSO: the full instantiations whose outputs have step stride 0 write them in the launch's LAST step only -- every earlier row would be overwritten
    // before anyone could read it (include/ev2g.h: the buffer holds the launch's last step; its contents while the launch runs are unspecified)
    constexpr bool LSO = FULL && !STR;
    constexpr bool INL = FULLK == 2 && !IO32 && !ACT && BLOCK == EV2G_WAVE_BLOCK;   // the in-launch statistics phase is compiled in (end of the kernel)
#if defined(EV2G_PHASE_TIMING) && defined(EV2G_PT_OUTER)
    const unsigned long long pt_k0 = __builtin_readcyclecounter();   // slot 7 := prologue, slot 6 := epilogue (tools/phase_timing.py --outer)
#endif
    typedef const V2P __attribute__((address_space(4))) *ParamPtr;
    ParamPtr S = (ParamPtr)(unsigned long long)params;
    constexpr int NS = BLOCK;
    constexpr int RS = NS + 8;   // stage row stride: +16 banks per row, so the 8 rows one reduction read touches spread over all banks
    const int P = wa.P, T = wa.T, E = wa.E, D = wa.D, M = wa.M;
    int off = io.scn_off;   // scenario-pool window: env e runs scenario (e + off) mod M
    // state slabs (ev2g_device.h): every [E*P] array is slabP + k * PS8, the three [T,E] histories slabH + k * HS8, the
    // two per-session result arrays slabS + k * SS8 -- scalar adds on three base pointers instead of one pointer fetch
    // from the parameter block per array and use
    const gptr slabP = (gptr)wa.slab_port, hist = (gptr)wa.hist, slabS = (gptr)S->slab_sess;
    const unsigned long long PS8 = wa.slab_port_slice, SS8 = S->sess_slice;
    const gptr env_acc = (gptr)wa.env_acc;
#define PA(k) (slabP + PS8 * (unsigned long long)(k))
    // envs per wavefront.  The fused instantiation gives EVERY env a wavefront of its own, whatever its width (a policy row is an env: 16 rows per
    // workgroup; the step's time is a chain of latencies, not lanes): the lanes behind the env's last port only copy observation-head pairs
    const int EPW = ACT ? AE : wa.epw;
    const int ES = ACT ? (AE == 1 ? P : 32) : wa.es;      // lanes from one env of the wavefront to the next
    const int G = (BLOCK / 64) * EPW;    // envs per workgroup
    int grp;
    {   // XCD-aware mapping: workgroup b runs on XCD b % 8; give each XCD a contiguous range of env groups
        const int nb = gridDim.x, b = blockIdx.x, per = nb >> 3;
        grp = (nb & 7) == 0 ? (b & 7) * per + (b >> 3) : b;
    }
    // CU balance (ev2g_balance_host.h): a fast-forwarding launch from step 0 is handed a permutation of the groups that puts heavy and light ones on one
    // CU -- only the instantiations that fast-forward (FFW below) look at it, the others are what they were; everything past e0 is indexed by env
    if (F64 && LSO && !ACT && RK != 3 && SK != 1 && BLOCK == EV2G_WAVE_BLOCK && wa.grp_map != nullptr) grp = wa.grp_map[blockIdx.x];
    const int e0 = grp * G;
    double *stage = lds;                                   // [NQ][RS] per-port step results, by home index (= tid)
    double *s_cap = stage + (size_t)EV2G_NQ * RS;
    double *s_tot = s_cap + NS, *s_prev = s_tot + NS, *s_bcap = s_prev + NS, *s_potc = s_bcap + NS;
    double *s_amps = s_potc + NS, *s_abse = s_amps + NS;
    double *eacc = s_abse + NS;                            // [G][7] episode accumulators + charge_power_potential[t], [t-1], per env
    double *s_cst = eacc + 7 * G;                          // [4][64] per-charger gates and clamps (rarely changing operands
                                                           // kept out of the register file): imin-0.01, dmin, max power, min power
    int *s_ta = (int *)(s_cst + 4 * 64);
    int *s_td = s_ta + NS, *s_ss = s_td + NS, *s_cyc = s_ss + NS, *s_dirty = s_cyc + NS, *items = s_dirty + NS;
    int *cnt = items + NS;  // cnt[2*(kk&1) + {0 charge, 1 discharge}]
    // Full kernels keep window, battery size and potential term in registers (below): the LDS behind s_bcap / s_potc / s_ta + s_td holds the attached
    // EV's transition_soc and efficiencies instead -- what the battery maths used to fetch from the session's own record -- and bits 20..31 of
    // s_dirty its dictionary entry (bits 8..19 the efficiency-table id + 1: a full kernel needs n_lut <= 4094, checked by the host)
    double *s_ts = s_bcap, *s_etac = s_potc, *s_etad = (double *)s_ta;
    constexpr int LUTMASK = FULL ? 0xfff : 0xffff;
    // ACT: the policy's input rows (bf16; env w of the workgroup = wavefront w = row w) and its actions behind the step's own LDS; its hidden
    // activations in the staging rows, which are dead between the end of a step and the next phase A (idle lanes re-zero their slots afterwards)
    // (round 6: PublicPST -- 3 + 3 P <= 63 inputs, P <= 20 outputs -- rides the 64 -> 400 -> 300 -> 32 packing: a third of layer 1's weight stream)
    typedef typename std::conditional<SK == 1, MlpS16<2, 25, 19, 2, 1, 4, AE>, MlpS16<6, 25, 19, 4, 1, 4, AE>>::type MC;
    constexpr int FSX = MC::SX;          // bf16 elements per observation row in LDS
    constexpr int FKS1 = (SK == 1) ? 2 : 6, FNT3 = (SK == 1) ? 2 : 4;
    uint16_t *bufX = (uint16_t *)(cnt + 8);
    float *lbias = (float *)(bufX + 16 * EV2G_FUSED_SX);   // the three bias vectors (MC::NB floats), staged once per launch
    // the actions of env w: the first 64 floats of wavefront w's own slice of s_amps (dead between a step's phase C and the next phase A; the
    // wavefront reads its actions -- one instruction, all lanes -- before it writes the amps over them)
    float *act_lds = (float *)s_amps;
    uint16_t *bufH1 = (uint16_t *)stage, *bufH2 = bufH1 + 16 * AE * MC::SH1;
    // NWF = 2: float32 input rows in bufX's place (no staged biases); H1's three copies, then two of H2's in the staging rows, H2's third over the input rows
    constexpr int FSXF = EV2G_FUSED_SXF;
    float *bufXf = (float *)(cnt + 8);
    static_assert(NWF == 1 || (3 * 16 * MC::SH1 * 2 <= 5 * RS * 8 && EV2G_NQ == 8 && FKS1 * 32 <= 256), "the input rows' bf16 terms live in staging rows 5..7, behind H1's three copies");
    static_assert(NWF == 1 || (FKS1 * 32 + 4 <= FSXF && (3 * MC::SH1 + 2 * MC::SH2) * 16 * 2 <= EV2G_NQ * (EV2G_FUSED_BLOCK + 8) * 8 && MC::SH2 * 16 * 2 <= 16 * FSXF * 4), "float32 policy buffers");
    static_assert(AE * MC::SX <= EV2G_FUSED_SX && MC::NB <= (25 + 19 + 4) * 16 && 16 * AE * (MC::SH1 + MC::SH2) * 2 <= EV2G_NQ * (EV2G_FUSED_BLOCK + 8) * 8, "policy buffers");
    constexpr int ACT_AS = (AE == 1) ? 128 : 64;   // floats between two envs' action rows in s_amps (a wavefront's slice holds its envs' rows)
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const bool log_soc = WIDE ? true : (S->soc_log != nullptr);
    const bool log_cs = FULL ? false : (S->cs_profits != nullptr);   // EV2G_FLAG_LOG_CS_HISTORY: charger-level accumulators and histories (ev2gym_env.py:533-535)
    const double dtd = (double)S->dt, sixty_over_dt = S->sixty_over_dt, dt_over_60 = S->dt_over_60;
    const bool pow2_dt = S->pow2_dt != 0;

    // FFW: EV-free stretches of a stride-0 float64 launch are fast-forwarded (below, behind the step's first barrier).  A step in which no port of
    // the workgroup's envs holds an EV or receives one writes nothing but three history words and the reward's share of the episode return, all of
    // them functions of the step's own step-table row: a stretch of n such steps is ONE pass with lane = step instead of n trips round the loop.
    // Every wavefront tells the others through LDS how long ITS env stays EV-free (ffx: 16 bits per wavefront, relative to the step in work,
    // double-buffered by step parity like cnt); n is the minimum of the four values, read by all wavefronts behind the same barrier, so the branch
    // -- and the barriers executed -- are the same in every wavefront of the workgroup by construction.
    // Off (ff_lim == 0) unless V2P::ff_count is set (EV2G_NO_FAST_FORWARD at load time), one env per wavefront, more than one step.  The launch's last
    // step always takes the normal path: it writes the outputs and publishes the accumulators.  (Phase-timing builds: compiled out.)
    // Not for PublicPST (SK 1): its benchmark shape, cfg3, runs three envs per wavefront and could never take the path, yet carrying it cost that kernel 3.5 %
    // (profiles/r15_ev_free_stretches.txt) -- every instantiation without the path is, instruction for instruction, what it was before.
#if defined(EV2G_PHASE_TIMING)
    constexpr bool FFW = false;
#else
    constexpr bool FFW = F64 && LSO && !ACT && RK != 3 && SK != 1 && BLOCK == EV2G_WAVE_BLOCK;
#endif
    unsigned short *ffx = (unsigned short *)(cnt + 4);   // [2][4]
    // (both wave-uniform, but kept in VECTOR registers: the scalar registers of these instantiations are spoken for, and one parked there is a
    // v_readlane / v_writelane pair in every step)
    int ff_lim_v = 0;    // index of the launch's last step; 0: no fast-forward in this launch
    int ff_next_v = -1;  // the step in which this wavefront's env is next live (== t while it is); recomputed only behind a live step
    if (FFW && EPW == 1 && k_steps > 1 && S->ff_count != nullptr) {   // (uniform)
        ff_lim_v = k_steps - 1;
        // this workgroup's count (bits 0..31 steps, 32.. stretches), cleared here: the prologue's wait below completes the store before the first addition
        if (tid == 0) stg32<unsigned long long>(S->ff_count, (unsigned)blockIdx.x * 8u, 0ull);
        if (tid == 0 && S->place != nullptr) {   // EV2G_PLACEMENT=1 at load time (development): the CU this workgroup runs on and its arrival rank there
            const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_REG_HW_ID, HW_REG_XCC_ID
            const unsigned cu = ((xcc & 7u) << 8) | ((hw >> 8) & 0xffu);   // XCC | SE | SH | CU: < 2048, the counters behind the 2 * gridDim.x words of the workgroups
            const unsigned rank = __hip_atomic_fetch_add(S->place + 2u * gridDim.x + cu, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            S->place[2u * blockIdx.x] = (xcc << 16) | (hw & 0xffffu);
            S->place[2u * blockIdx.x + 1u] = rank;
        }
    }
    // launch stamps: the wide stride-0 instantiations (FULLK 2: a whole-episode launch's) read the wall clock at both ends of the kernel when the host
    // passes a pair (WaveArgs::stamp; timing_wave_stamped in ev2g_timing_host.h is the rule, which route_step applies as StepRoute::stamps on the host).  Only they: their peeled step keeps the kernel-argument
    // pointer alive across the loop anyway, so the end site costs them nothing, while every other instantiation paid for it with scalar registers parked
    // in lanes and the general one with 68 bytes of scratch (profiles/r28_launch_stamps.txt)
    constexpr bool STAMPED = timing_wave_stamped(FULLK) && !ACT && BLOCK == EV2G_WAVE_BLOCK;
    if (STAMPED && blockIdx.x == 0 && tid == 0) {
        unsigned long long *stamp = ev2g_wave_stamp_arg();
        if (stamp != nullptr) stamp[0] = wall_clock64();
    }
    // ---- home lane set-up ----
    const int elw = lane / ES;           // env inside the wavefront
    const int q = (ACT && AE == 1) ? lane : lane - elw * ES;       // port slot (== reference port: one transformer, single-port chargers)
    const int e = (ACT && AE == 1) ? e0 + wv : e0 + wv * EPW + elw;
    const bool valid = (elw < EPW) && (q < P) && (e < E);
    const bool hcopy = ACT && AE == 1 && !valid && e < E && lane < 32;   // (ACT, envs narrower than their head pairs: lanes P .. NPAIR-1 copy the pairs the ports cannot)
    const int g = valid ? e * P + q : 0;
    const int ocol = (SK == 1) ? 3 + 3 * q : (SK == 0 ? 62 + 2 * q : 22 + 2 * q);
    const int cs = valid ? q : 0;
    int t = t0;
    const bool head = valid && q == 0;   // one lane per env: env-level scalars
    const int elg = wv * EPW + elw;      // env inside the workgroup
    const int arow = (AE == 1) ? wv : min(elg, 16 * AE - 1);   // (ACT) this lane's env as a row of the policy's buffers
    // the policy's copy of an observation column pair (even column): packed bf16, or the float32 values themselves
    auto xput2 = [&](int col, float a, float b) __attribute__((always_inline)) {
        if (NWF > 1) *(float2 *)(bufXf + arow * FSXF + col) = make_float2(a, b);
        else *(uint32_t *)(bufX + arow * FSX + col) = ev2g_pack_bf16(a, b);
    };
    // ---- launch prologue.  A single-step launch (the RL loop with a policy between steps) pays it every step, with cold caches.
    // Round trip 1: what does not depend on data -- charger constants, the first action, the env accumulators and, for a single-step launch,
    // the scenario's occupancy / arrival masks of this step (step table slots 6, 7: occupancy does not depend on the actions); for a longer
    // launch the head chunk of every port's state line instead.  Round trip 2: the state lines (PortLine, 64 bytes = one sector) of the
    // ports that hold an EV -- in a single-step launch also the head chunk, and only for ports that hold an EV or receive one this step.
    double c_imax, c_dmaxabs, a_next;
    // FULL kernels keep what only the port's own lane touches -- its occupancy window, the attached EV's battery size and potential
    // term -- in registers instead of LDS (no in-launch reset rewrites them from outside): six LDS instructions a step less
    int r_ta = EV2G_INT_MAX, r_td = -1;
    double r_bcap = 1.0, r_potc = 0.0;
    double r_rb = 1.0;   // RN(1 / battery size) of the attached EV: the observation's cap / B goes through it (ev2g_fdiv2) in the full kernels
    const unsigned l64 = (unsigned)g * (unsigned)sizeof(PortLine);   // this port's state line
    static_assert(sizeof(PortLine) == 64 && offsetof(PortLine, cap) == 16 && offsetof(PortLine, prev) == 32 && offsetof(PortLine, bcap) == 48, "PortLine layout");
    {
        const unsigned c8 = (unsigned)cs * 8u, cp8 = (unsigned)min(tid, P - 1) * 8u;
        const unsigned ec = (unsigned)(valid ? e : e0);
        const bool by_mask = (k_steps == 1) && (t < T);   // (uniform)
        i4v hd = {EV2G_INT_MAX, -1, -1, 0};                // {t_arr, t_dep, session, cycles | table id + 1}
        d2v mk = {0.0, 0.0};
        if (by_mask) mk = ldg32<d2v>(wa.step_tab, (unsigned)(ev2g_scn((int)ec, off, M) * T + t) * 64u + 48u);
        else hd = ldg32<i4v>(wa.lines, l64);
        const d2v k_max = ldg32<d2v>(wa.cs_pack, c8 * 6u);   // (imax, |dmax|) of this lane's charger
        d2v k_min = {0.0, 0.0}, k_pow = {0.0, 0.0};            // gates and clamps, staged in LDS by the first P lanes of the workgroup
        if (tid < 64) { k_min = ldg32<d2v>(wa.cs_pack, cp8 * 6u + 16u); k_pow = ldg32<d2v>(wa.cs_pack, cp8 * 6u + 32u); }   // (wavefront 0 only)
        if (ACT) a_next = 0.0;   // (the policy runs inside the launch: its actions arrive through LDS)
        else
        a_next = IO32 ? (double)ldg32<float>(io.act32 + (long long)io.step0 * io.a_stride, (unsigned)(valid ? g : e0 * P) * 4u)
                      : ldg32<double>(io.actions, (unsigned)(valid ? g : e0 * P) * 8u);
        double l_pot = ldg32<double>(hist, ((ec * (unsigned)T + (unsigned)min(t, T - 1)) * 3u + 1u) * 8u);
        double l_pot2 = 0.0;   // charge_power_potential[t-1]: only SquaredTrackingErrorRewardWithPenalty (a run-time reward) reads it
        if (RK == 3) l_pot2 = ldg32<double>(hist, ((ec * (unsigned)T + (unsigned)min(max(t - 1, 0), T - 1)) * 3u + 1u) * 8u);
        d2v acc01 = ldg32<d2v>(env_acc, ec * 64u), acc23 = ldg32<d2v>(env_acc, ec * 64u + 16u);
        double acc4 = ldg32<double>(env_acc, ec * 64u + 32u);
        d2v k_max_w = k_max;
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(hd), "+v"(mk), "+v"(k_max_w), "+v"(k_min), "+v"(k_pow),
                     "+v"(a_next), "+v"(l_pot), "+v"(l_pot2), "+v"(acc01), "+v"(acc23), "+v"(acc4));
        c_imax = k_max_w.x; c_dmaxabs = k_max_w.y;
        if (tid < P) {
            s_cst[0 * 64 + tid] = k_min.x - 0.01; s_cst[1 * 64 + tid] = k_min.y;
            s_cst[2 * 64 + tid] = k_pow.x; s_cst[3 * 64 + tid] = k_pow.y;
        }
        if (valid) {
            bool body;   // an EV is attached in the launch's first step: the rest of the line is needed
            if (by_mask) {
                const unsigned long long m_occ = (unsigned long long)__double_as_longlong(mk.x), m_arr = (unsigned long long)__double_as_longlong(mk.y);
                body = (m_occ >> q) & 1ull;
                if (body || ((m_arr >> q) & 1ull)) hd = ldg32<i4v>(wa.lines, l64);   // (a port without either keeps the defaults: no event can touch it this step)
            } else body = (hd.x <= t) && (t <= hd.y);
            d2v b1 = {0.0, 0.0}, b2 = {0.0, 0.0}, b3 = {1.0, 0.0};
            d2v pd0 = {1.0, 1.0}; i4v pd1 = {0, 0, -1, 0};
            static_assert(sizeof(PortDyn) == 32 && offsetof(PortDyn, eta_dis) == 16 && offsetof(PortDyn, lut) == 24 && offsetof(PortDyn, cls) == 28, "PortDyn layout");
            if (body) {
                b1 = ldg32<d2v>(wa.lines, l64 + 16u); b2 = ldg32<d2v>(wa.lines, l64 + 32u); b3 = ldg32<d2v>(wa.lines, l64 + 48u);
                if (FULL) { pd0 = ldg32<d2v>(wa.port_dyn, (unsigned)g * 32u); pd1 = ldg32<i4v>(wa.port_dyn, (unsigned)g * 32u + 16u); }
            }
            r_ta = hd.x; r_td = hd.y;
            if (!FULL) { s_ta[tid] = hd.x; s_td[tid] = hd.y; }
            s_ss[tid] = hd.z; s_cyc[tid] = ev2g_line_cycles(hd.w);
            // s_dirty: bits 0,1 = what the epilogue must write back; bits 8..23 = 1 + efficiency-table id of the attached EV,
            // so that the battery maths can issue the table look-up together with (not behind) the session-record load
            s_dirty[tid] = (int)(((unsigned)hd.w >> 16) << 8 | ((FULL && wa.dict) ? (unsigned)pd1.w << 20 : 0u));
            if (FULL) { s_ts[tid] = pd0.x; s_etac[tid] = pd0.y; s_etad[tid] = __hiloint2double(pd1.y, pd1.x); }
            s_cap[tid] = b1.x; s_tot[tid] = b1.y; s_prev[tid] = b2.x; s_abse[tid] = log_soc ? b2.y : 0.0;
            r_bcap = b3.x; r_potc = b3.y;
            if (FULL) { if (body) r_rb = 1.0 / r_bcap; }
            else { s_bcap[tid] = r_bcap; s_potc[tid] = r_potc; }
        }
        if (head) {   // episode accumulators (continued from global memory) and charge_power_potential[t], in LDS
            double *ea = eacc + elg * 7;
            ea[0] = acc01.x; ea[1] = acc01.y; ea[2] = acc23.x; ea[3] = acc23.y; ea[4] = acc4;
            ea[5] = (t < T) ? l_pot : 0.0;
            ea[6] = (t > 0 && t <= T) ? l_pot2 : 0.0;
        }
    }
    if (tid < 4) cnt[tid] = 0;
    for (int k = 0; k < EV2G_NQ; k++) stage[k * RS + tid] = 0.0;
    if (ACT) {   // the observation the first forward reads (the reset observation, or the last step's of an earlier segment): this wavefront's env row -> bf16
        const bool env_ok = (e0 + arow) < E;   // (one env per wavefront; AE = 2: one per half)
        const float *xr = fa.obs0 + (long long)(env_ok ? e0 + arow : e0) * D;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int c = (AE == 1) ? 2 * lane + 128 * j : 2 * (lane & 31) + 64 * j;
            float2 v = make_float2(0.f, 0.f);
            if (SK == 1) {   // (D = 3 + 3 P may be odd: rows are 4-byte aligned only)
                if (env_ok && c < D) v.x = xr[c];
                if (env_ok && c + 1 < D) v.y = xr[c + 1];
            } else {
                if (env_ok && c + 1 < D) v = *(const float2 *)(xr + c);   // (D even: 22 + 40 + 2 P, 22 + 2 P)
                else if (env_ok && c < D) v.x = xr[c];
            }
            if (NWF > 1) { if (c < FKS1 * 32) xput2(c, v.x, v.y); }
            else
            if (c < FSX) *(uint32_t *)(bufX + arow * FSX + c) = ev2g_pack_bf16(v.x, v.y);   // columns D .. : zeros (the k-steps' padding)
        }
        if (NWF == 1 && tid < MC::NB) lbias[tid] = fa.m.b1[tid];   // (b1 | b2 | b3 are one array on this path, each padded to its tiles)
    }
    __syncthreads();

    // FULL kernels have registers to spare (no extras, no second head pair): what the step loop otherwise re-derives every step with
    // quarter-rate integer multiplies -- this lane's rows in the step / head tables (the scenario does not change: no in-launch reset)
    // and its places in the observation -- is computed once and kept
    unsigned hb_step = 0, hb_head = 0, hb_obs_port = 0, hb_obs_env = 0;
    const double *act_run = io.actions;   // the actions of the step in work
    const float *act32_run = (F32 && !ACT) ? io.act32 + (long long)io.step0 * io.a_stride : nullptr;
    double *obs_run = io.obs, *rew_run = io.reward;   // the outputs of the step in work (STR: advanced by their step strides; else the launch's one row)
    uint8_t *done_run = io.done, *mask_run = io.mask;
    float *obs32_run = io.obs32, *act_out = ACT ? const_cast<float *>(io.act32) + (long long)e0 * P : nullptr;   // (ACT: the rows the policy writes, this workgroup's first env)
    constexpr unsigned OB = F32 ? 4u : 8u;    // bytes per observation element the full kernel writes
    if (FULL) {
        const int scn0 = ev2g_scn((valid || hcopy) ? e : e0, off, M);
        hb_step = (unsigned)(scn0 * T) * 64u;
        hb_head = (unsigned)(scn0 * (T + 1)) * (unsigned)(((SK == 1) ? 0 : (SK == 0 ? 60 : 20)) * 8);
        hb_obs_env = (unsigned)(e * D) * OB;
        if (WIDE) hb_obs_port = hb_obs_env + (unsigned)ocol * OB;
    }
    PT_DECL
#if defined(EV2G_PHASE_TIMING) && defined(EV2G_PT_OUTER)
    pt_cur[7] += pt_last - pt_k0;
#endif
    // The step body (ev2g_step_wave_body.h) is compiled once per compile-time OUT: OUT says whether the step writes the observation / reward / done / mask rows.
    // The LSO instantiations run every step but the launch's last with OUT = false -- there the output stores, the head-table request and every register only
    // they use are not branched around but absent, and only that body carries the fast-forward path -- and the last one with OUT = true (k_steps == 1: that
    // body alone): one always-inlined callable around the body, instantiated twice.  All other instantiations write every step's rows and keep the body INSIDE
    // their loop, token for token the loop they always had: around the callable every one of them took another VGPR and PublicPST's strided one spilled 12
    // bytes to scratch (profiles/r27_step_loop.txt).
    if constexpr (!LSO) {
        constexpr bool OUT = true;
#define EV2G_STEP_SKIP(n) { kk += (n) - 1; continue; }
#define EV2G_STEP_BREAK break
        for (int kk = 0; kk < k_steps; kk++) {
#include "ev2g_step_wave_body.h"
        }
#undef EV2G_STEP_SKIP
#undef EV2G_STEP_BREAK
    } else {
        // (kk by value and the steps done as the return value: written through a reference next to t, the two ended up behind one pointer and in scratch)
        auto step = [&](auto outc, const int kk) __attribute__((always_inline)) -> int {
            constexpr bool OUT = decltype(outc)::value;
#define EV2G_STEP_SKIP(n) return (n)
#define EV2G_STEP_BREAK return 0
#include "ev2g_step_wave_body.h"
#undef EV2G_STEP_SKIP
#undef EV2G_STEP_BREAK
            return 1;
        };
        int kk = 0;
        while (kk < k_steps - 1) kk += step(std::false_type{}, kk);   // (a fast-forward pass stops short of the last step: kk <= k_steps - 1 behind the loop)
        if (kk < k_steps) {
            {   // the output pointers, fetched from the kernel arguments HERE: only this step uses them, and held from the prologue on they were scalar
                // registers parked in lanes across the whole loop
                typedef const StepIO __attribute__((address_space(4))) *IoPtr;
                static_assert(sizeof(params) == 8 && alignof(StepIO) == 8, "StepIO follows the parameter-block pointer in the kernel-argument segment");
                const char __attribute__((address_space(4))) *kargs = (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(kargs));
                IoPtr iop = (IoPtr)(kargs + 8);
                obs_run = iop->obs; rew_run = iop->reward; done_run = iop->done; mask_run = iop->mask; obs32_run = iop->obs32;
            }
            step(std::true_type{}, kk);
        }
    }
    __syncthreads();
    if (valid) {
        const int d = s_dirty[tid];
        const unsigned g8 = (unsigned)g * 8u;
        if (d & 3) stg32<i4v>(wa.lines, l64, (i4v){FULL ? r_ta : s_ta[tid], FULL ? r_td : s_td[tid], s_ss[tid], ev2g_line_pack(s_cyc[tid], ((d >> 8) & LUTMASK) - 1)});
        if (d & 1) {
            stg32<d2v>(wa.lines, l64 + 16u, (d2v){s_cap[tid], s_tot[tid]});
            stg32<d2v>(wa.lines, l64 + 32u, (d2v){s_prev[tid], s_abse[tid]});
        }
    }
#if defined(EV2G_PHASE_TIMING) && defined(EV2G_PT_OUTER)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PT_MARK(6)
#endif
    PT_FLUSH
    // ---- in-launch episode statistics (INL: the float64 wide instantiation) ----
    // A launch of more than one step that ends the episode (t == T) computes get_statistics into V2P::stats_inl -- set by the loader only for a shape
    // the statistics kernel runs one env per wavefront, like this phase (route_step in ev2g_route_host.h applies the same rule) -- for
    // for its own envs right here, while other workgroups are still stepping: everything the statistics read of env e -- its SoC log, history
    // rows, charger counters, state lines, per-session results and episode accumulators -- was written by this workgroup, and the barrier
    // below orders those stores (and the departures' atomics) before the loads.  Wavefront w computes env e0 + w with ev2g_env_stats, the
    // statistics kernel's code (bit-identical results); the step's LDS is dead by now and holds each wavefront's [LK][64] block of parked
    // SoC-log entries.  ev2g_get_stats / ev2g_get_stats_reset then copy the rows instead of recomputing them.
    // (nothing of this phase is kept live across the step loop: the scalar registers of the full kernels are spoken for -- its pointers come from
    // the parameter block, the env's scenario from this lane's step-table row)
    double *stats_out = (INL && t == T && k_steps > 1) ? (double *)S->stats_inl : nullptr;
    if (stats_out != nullptr) {   // (uniform)
        __syncthreads();   // the epilogue's LDS reads are done; this workgroup's global stores and atomics are visible to all of its wavefronts
        const int es = e0 + wv;
        if (es < S->E) {   // (then lane 0 holds port 0 of env es: its step-table row is that of the env's scenario)
            const int scn_s = (int)(__builtin_amdgcn_readfirstlane(hb_step) / (64u * (unsigned)T));
            StatsView v{T, S->C, S->R, P, S->dt, (const double *)S->setpoint, (const int *)S->scn_sess, (const int *)S->scn_sess_end,
                        (const int *)S->ss_slot, (const int *)S->ss_tarr, (const int *)S->ss_tdep, (const double *)S->ss_B, (const double *)S->ss_afap,
                        (const int *)S->cs_served, (const double *)S->cs_sat_sum, (const double *)S->hist, (const double *)S->env_acc,
                        (const double *)S->sess_final_cap, (const double *)S->sess_abs_e, (const double *)S->soc_log, (const PortLine *)S->line};
            ev2g_env_stats<1, EV2G_INL_STATS_NK, EV2G_INL_STATS_LK>(v, es, true, scn_s, lane, T, stats_out,
                                                                  lds + (size_t)wv * EV2G_INL_STATS_LK * 64, lane);
        }
    }
    // the launch's end stamp: every workgroup's exit time -- read behind a barrier, so it is its last wavefront's --, the largest one stays (relaxed,
    // result unused: no round trip; the clock only grows, so a pair reused by a later launch needs no clearing).  ONE atomic per workgroup: an agent-scope
    // atomic executes at the memory side, those on one word queue up there, and a balanced launch's workgroups end together -- one per wavefront (4096 at
    // cfg2) made the cfg2 headline 3.2 % SLOWER than the parent, one per workgroup measures like none at all (profiles/r28_launch_stamps.txt)
    // Which wavefront issues it: the first one behind the barrier to swap a marker into cnt[0] -- dead since the step loop, never negative (a count of
    // ports), and beyond the statistics phase's LDS blocks.  (`tid == 0` instead kept the thread index alive to the end: two VGPRs more.)
    static_assert(!STAMPED || (size_t)BLOCK * EV2G_INL_STATS_LK * sizeof(double) <=sizeof(double) * (EV2G_NQ * (size_t)RS + 7 * (size_t)NS + 4 * 64) + sizeof(int) * 6 * (size_t)NS, "the statistics phase's blocks end in front of cnt");
    // A launch without a pair (the one-step launches of a chain) skips all of it behind one scalar load: the barrier and the swap cost such a 10 us
    // launch 0.7 %, the load and its wait still cost it 0.3-0.4 % (profiles/r28_launch_stamps.txt section 3).
    if (STAMPED) {
        unsigned long long *stamp = ev2g_wave_stamp_arg();
        if (stamp != nullptr) {   // (uniform: a kernel argument)
            __syncthreads();
            if (lane == 0 && __hip_atomic_exchange(cnt, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != -1)
                __hip_atomic_fetch_max(stamp + 1, (unsigned long long)wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
