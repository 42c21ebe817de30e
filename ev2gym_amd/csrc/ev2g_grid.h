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
    for (int i = lane; i < n; i += 64) {
        const double2 a = v[i];
        const double m = ev2g_grid_abs(a);
        const double x = 0.05 - fabs(1.0 - m);
        loss += (x < 0.0 || x != x) ? x : 0.0;   // np.minimum(0, x): a NaN stays
        if (g.vm) g.vm[(long long)row * (n + 1) + 1 + i] = m;
        if (g.vc) { g.vc[((long long)row * n + i) * 2] = a.x; g.vc[((long long)row * n + i) * 2 + 1] = a.y; }
    }
    for (int m = 32; m >= 1; m >>= 1) loss += __shfl_xor(loss, m);
    if (lane == 0) {
        if (g.vm) g.vm[(long long)row * (n + 1)] = 1.0;
        if (g.iters) g.iters[row] = it;
        if (g.loss) g.loss[row] = loss;
        if (COMPOSE && g.reward) {
            const double lv = g.voltage_weight * loss;
            g.reward[row] = (g.base_weight == 0.0) ? lv : g.base_weight * g.reward[row] + lv;
        }
    }
}
