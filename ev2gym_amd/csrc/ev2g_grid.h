// ev2g_grid.h -- the reference's distribution-grid power flow (ev2gym/models/grid.py:120-199, grid_utility/grid_tensor.py:559-711) on the
// device, after a one-step launch of the step kernel (the pattern of ev2g_heuristic.h / ev2g_link.h: no step kernel changes).
//   ev2g_grid_kernel<COMPOSE>  a batched constant-power Laurent power flow: one wavefront per row (env).  With S = (P + jQ) / s_base over the
//           n = n_bus - 1 non-slack buses and a flat start v = 1 + 0j it repeats
//               lambda = conj(S * (1 / v));   v' = K lambda + L;   tol = max_i | |v'_i| - |v_i| |;   v = v'
//           while iterations < max_iter and tol >= tolerance (power_flow_tensor_constant_power with ts = 1: the stopping rule is PER ROW).
//           A row is a wavefront, so a row that has converged simply leaves its loop: its v and its iteration count are final while the other
//           rows of the workgroup go on (no workgroup barrier anywhere in the kernel).  The loop counts to max_iter whatever the data does; a
//           NaN residual ends it at once, as numpy's `nan >= tolerance` does.
//           Lane i owns bus i, i + 64, ...: it keeps v_i in LDS, writes lambda_i there, and sums row i of K lambda over j = 0 .. n - 1 in that
//           order with fused multiply-adds (numpy's product goes through BLAS, whose order is not defined: parity is by tolerance).  K is stored
//           TRANSPOSED (Kt[j, i] = K[i, j]) so that the lanes of a wavefront read consecutive 16-byte words; for 123 buses it is 238 KB, read
//           through L2 by every wavefront; lambda_j is an LDS broadcast.
//           Outputs per row: |v| with the slack's 1.0 in front [n_bus]; optionally v [n, 2]; the iteration count; the voltage loss
//           sum_i min(0, 0.05 - |1 - |v_i||) over all n_bus entries (rl_agent/reward.py:117-119).
//           COMPOSE (ev2g_grid_run, after step t of env e): P_i = P_base[scenario, t, i] + tr_power_now[e, i] (PowerGrid.step: active_power +=
//           actions; ev2gym_env.py:388-393: node i + 1 carries transformer i's current_power), Q_i = Q_base[scenario, t, i], and
//           reward[e] = base_weight * reward[e] + voltage_weight * loss_v (base_weight == 0: the step's reward is not read).
//           COMPOSE also keeps the episode's voltage statistics (get_statistics, utilities/utils.py:65-112) per env, in the same epilogue pass
//           that holds every |v_i| in a register: vv_sum += loss_v, vv_count += #{|v_i| < 0.95} + #{|v_i| > 1.05} over the n non-slack buses
//           (the slack's 1.0 never counts), vv_steps += (that count > 0), rew_sum += the composed reward.  One more wavefront reduction (the
//           count) and lane 0's four read-modify-writes; a launch with t == 0 overwrites instead of adding, so an episode restarts them itself.
//   ev2g_grid_state_kernel     the reference's V2G_grid_state row (rl_agent/state.py:216-278) of every env for step counter c, 0 <= c <= T:
//               [weekday/7, sin(hour), cos(hour) | charge price[c] (signed) | setpoint[c] | usage[c-1] | P_base[c, :] | Q_base[c, :] |
//                per port in reference port order (current_capacity, time_of_departure - c + 1, connected_bus) or three zeros]
//           Dg = 6 + 2 n + 3 P columns.  ONE LANE PER OUTPUT ELEMENT in the row's order (a grid-stride loop over E * Dg): consecutive lanes
//           write consecutive words of the float64 and float32 blocks and read consecutive words of P_base / Q_base, which are two thirds of
//           a row on the feeders this was written for; the three lanes of a port read the same 64-byte PortLine (one sector).  Every entry
//           is a copy, an integer difference or a constant -- no floating-point arithmetic, so the row is the reference's bit for bit; the
//           float32 block is the plain (float) conversion.  A port holds an EV exactly when ev2g_heur_port says so for t = c.
// Differences to the reference: one row per wavefront means every env stops on ITS residual (the reference solves one env at a time, so this is
// its rule; a numpy call with ts > 1 would stop all rows on the batch's worst one).
#pragma once
#include "ev2g_heuristic.h"

#define EV2G_GRID_WAVES 4
#define EV2G_GRID_LDS_MAX 49152   // dynamic LDS of a workgroup: what a launch may ask for without hipFuncSetAttribute

// LDS bytes of one row's stage: S, v and lambda, n complex128 each
__host__ __device__ inline size_t ev2g_grid_wave_bytes(int n) { return (size_t)n * 48; }

struct GridArgs {
    const double2 *Kt;   // [n, n] K transposed
    const double2 *L;    // [n]
    int n;               // n_bus - 1
    int max_iter;
    double s_base, tolerance;
    // the rows' powers in kW: plain [n_rows, n] arrays, or (COMPOSE) the base profiles [M, T + 1, n] plus the transformers' power [E, n]
    const double *p, *q;
    const double *tr_power;
    int M, T1, t, scn_off;
    int n_rows;
    // outputs (each may be nullptr)
    double *vm;          // [n_rows, n + 1]
    double *vc;          // [n_rows, n, 2]
    int *iters;          // [n_rows]
    double *loss;        // [n_rows]
    double *reward;      // [n_rows] (COMPOSE)
    double base_weight, voltage_weight;
    // the episode's voltage statistics [n_rows] each (COMPOSE; all four or none: nullptr for ev2g_grid_solve)
    double *vv_sum, *rew_sum;
    int *vv_count, *vv_steps;
};

// |a + jb| as numpy's abs of a complex128 (hypot)
__device__ __forceinline__ double ev2g_grid_abs(double2 z) { return hypot(z.x, z.y); }

template <bool COMPOSE>
__global__ void __launch_bounds__(64 * EV2G_GRID_WAVES) ev2g_grid_kernel(GridArgs g) {
    extern __shared__ double2 ev2g_grid_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + wave;
    if (row >= g.n_rows) return;   // (a whole wavefront: nothing below synchronises across wavefronts)
    const int n = g.n;
    double2 *S = ev2g_grid_lds + (size_t)wave * 3 * n, *v = S + n, *lam = v + n;
    {
        const double *p, *q, *tr = nullptr;
        if (COMPOSE) {
            const long long scn = ((long long)row + g.scn_off) % g.M;
            const long long o = (scn * g.T1 + g.t) * n;
            p = g.p + o; q = g.q + o; tr = g.tr_power + (long long)row * n;
        } else {
            p = g.p + (long long)row * n; q = g.q + (long long)row * n;
        }
        for (int i = lane; i < n; i += 64) {
            const double pi = COMPOSE ? p[i] + tr[i] : p[i];
            S[i] = make_double2(pi / g.s_base, q[i] / g.s_base);
            v[i] = make_double2(1.0, 0.0);
        }
    }
    ev2g_wave_sync();
    int it = 0;
    double tol = __builtin_inf();
    while (it < g.max_iter && tol >= g.tolerance) {
        for (int i = lane; i < n; i += 64) {
            // 1 / v (numpy's complex reciprocal up to rounding), S * that, conjugated
            const double2 a = v[i], s = S[i];
            const double d = a.x * a.x + a.y * a.y;
            const double rx = a.x / d, ry = -a.y / d;
            lam[i] = make_double2(s.x * rx - s.y * ry, -(s.x * ry + s.y * rx));
        }
        ev2g_wave_sync();
        double worst = 0.0;
        bool bad = false;
        for (int i = lane; i < n; i += 64) {
            const double2 *k = g.Kt + i;
            double zr = 0.0, zi = 0.0;
#pragma unroll 4
            for (int j = 0; j < n; j++) {
                const double2 kk = k[(size_t)j * n], l = lam[j];
                zr = __builtin_fma(kk.x, l.x, zr); zr = __builtin_fma(-kk.y, l.y, zr);
                zi = __builtin_fma(kk.x, l.y, zi); zi = __builtin_fma(kk.y, l.x, zi);
            }
            const double2 li = g.L[i];
            const double2 nv = make_double2(zr + li.x, zi + li.y);
            const double r = fabs(ev2g_grid_abs(nv) - ev2g_grid_abs(v[i]));
            bad = bad || r != r;
            worst = (r > worst) ? r : worst;
            v[i] = nv;   // (v_i is read by its own lane only)
        }
        for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(worst, m); worst = (o > worst) ? o : worst; }
        tol = (__ballot(bad) != 0ull) ? __builtin_nan("") : worst;   // np.max propagates a NaN
        it += 1;
        ev2g_wave_sync();   // lambda is rewritten next
    }
    // |v| with the slack bus in front, and the voltage loss over all n_bus entries (the slack's term is min(0, 0.05) = 0)
    double loss = 0.0;
    int out_of_band = 0;   // (COMPOSE) buses outside 0.95 .. 1.05 p.u., utils.py:73
    for (int i = lane; i < n; i += 64) {
        const double2 a = v[i];
        const double m = ev2g_grid_abs(a);
        const double x = 0.05 - fabs(1.0 - m);
        loss += (x < 0.0 || x != x) ? x : 0.0;   // np.minimum(0, x): a NaN stays
        if (COMPOSE) out_of_band += (m < 0.95) + (m > 1.05);
        if (g.vm) g.vm[(long long)row * (n + 1) + 1 + i] = m;
        if (g.vc) { g.vc[((long long)row * n + i) * 2] = a.x; g.vc[((long long)row * n + i) * 2 + 1] = a.y; }
    }
    for (int m = 32; m >= 1; m >>= 1) loss += __shfl_xor(loss, m);
    if (COMPOSE && g.vv_sum)
        for (int m = 32; m >= 1; m >>= 1) out_of_band += __shfl_xor(out_of_band, m);
    if (lane == 0) {
        if (g.vm) g.vm[(long long)row * (n + 1)] = 1.0;
        if (g.iters) g.iters[row] = it;
        if (g.loss) g.loss[row] = loss;
        if (COMPOSE && g.reward) {
            const double lv = g.voltage_weight * loss;
            const double r = (g.base_weight == 0.0) ? lv : g.base_weight * g.reward[row] + lv;
            g.reward[row] = r;
            if (g.vv_sum) g.rew_sum[row] = (g.t == 0) ? r : g.rew_sum[row] + r;
        }
        if (COMPOSE && g.vv_sum) {
            const bool first = g.t == 0;   // a new episode: overwrite
            g.vv_sum[row] = first ? loss : g.vv_sum[row] + loss;
            g.vv_count[row] = first ? out_of_band : g.vv_count[row] + out_of_band;
            g.vv_steps[row] = (first ? 0 : g.vv_steps[row]) + (out_of_band > 0 ? 1 : 0);
        }
    }
}

#define EV2G_GRID_STATE_BLOCK 256

struct GridStateArgs {
    const double *tf;        // [M or 1, T + 1, 3] weekday / 7, sin, cos of sim_date at every step counter
    int tf_per_scn;          // 0: one table for every scenario
    const double *p, *q;     // [M, T + 1, n] the grid's base profiles
    int n;                   // n_bus - 1
    int c;                   // the step counter, 0 .. T
    int Dg;                  // 6 + 2 n + 3 P
    double *obs;             // [E, Dg] or nullptr
    float *obs32;            // [E, Dg] or nullptr
};

__global__ void __launch_bounds__(EV2G_GRID_STATE_BLOCK) ev2g_grid_state_kernel(DevScn s, DevState st, HeurArgs a, GridStateArgs g) {
    const long long total = (long long)s.E * g.Dg;
    const int T = s.T, n = g.n, c = g.c;
    for (long long i = (long long)blockIdx.x * EV2G_GRID_STATE_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * EV2G_GRID_STATE_BLOCK) {
        const int e = (int)(i / g.Dg), col = (int)(i - (long long)e * g.Dg);
        const long long scn = ((long long)e + a.scn_off) % s.M;
        double v;
        if (col < 3) {
            v = g.tf[((g.tf_per_scn ? scn : 0) * (T + 1) + c) * 3 + col];
        } else if (col == 3) {
            v = (c < T) ? s.price_ch[scn * T + c] : 0.0;       // charge_prices[0, c:c+1], padded with a zero at the end
        } else if (col == 4) {
            v = (c < T) ? s.setpoint[scn * T + c] : 0.0;
        } else if (col == 5) {
            v = (c > 0) ? st.hist[EV2G_HIST(e, c - 1, T, s.R)] : 0.0;   // current_power_usage[-1] of a freshly zeroed array
        } else if (col < 6 + n) {
            v = g.p[(scn * (T + 1) + c) * n + (col - 6)];
        } else if (col < 6 + 2 * n) {
            v = g.q[(scn * (T + 1) + c) * n + (col - 6 - n)];
        } else {
            const int k = col - 6 - 2 * n, p = k / 3, f = k - 3 * p;
            int slot, t_dep;
            double cap;
            const int ss = ev2g_heur_port(s, st, a, e, p, c, slot, cap, t_dep);
            v = (ss < 0) ? 0.0 : (f == 0) ? cap : (f == 1) ? (double)(t_dep - c + 1) : (double)s.slot_tr[slot];
        }
        if (g.obs) g.obs[i] = v;
        if (g.obs32) g.obs32[i] = (float)v;
    }
}

// float64 copy of a float32 block (the policy's actions of ev2g_grid_rollout, widened as the engine widens float32 actions on entry): the
// mirror of ev2g_link_f32_kernel
__global__ void __launch_bounds__(EV2G_GRID_STATE_BLOCK) ev2g_grid_widen_kernel(const float *__restrict__ src, double *__restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * EV2G_GRID_STATE_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * EV2G_GRID_STATE_BLOCK) dst[i] = (double)src[i];
}
