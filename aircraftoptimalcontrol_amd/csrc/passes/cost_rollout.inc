// passes/cost_rollout.inc — stored cost, nonlinear rollout with cost, the P-controller initial guess.
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// pass-level kernels: one wavefront per tile
// ---------------------------------------------------------------------------------------------

// cost of a stored trajectory, t ascending then terminal (optcon.py:417-424)
template <bool DIAG, bool RPT, typename XT>
__global__ __launch_bounds__(TILE) void k_traj_cost(KConst k, const real* __restrict__ ref,
                                                    const XT* __restrict__ x, const real* __restrict__ u,
                                                    const real* __restrict__ x0, real* __restrict__ J) {
    const int tile = blockIdx.x, lane = threadIdx.x, T = k.T;
    real JJ = R(0.0), xs[6], q[6], r[2], rb[8];
    for (int t = 0; t < T - 1; t++) {
        load_state(x, x0, tile, T, t, lane, xs);
        const real u0 = u[tix<2>(tile, T, t, 0, lane)], u1 = u[tix<2>(tile, T, t, 1, lane)];
        JJ += stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, t, rb), q, r);
    }
    load_state(x, x0, tile, T, T - 1, lane, xs);
    JJ += term_cost2<DIAG>(k, xs, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
    J[tile * TILE + lane] = R(0.5) * JJ;  // JJ accumulated twice the cost, see stage_cost2
}

// One nonlinear rollout with cost for per-lane step `a` (get_update + trial cost).
// WRITE: store x',u'.  wmask: lane writes only if true.
// The multi-wavefront kernels of small batches keep their uniform constants in VGPRs (pin_consts, aoc_device.h):
// `k` is the pinned copy of the kernel argument `kc`, `tk` the sin/cos coefficients.
#ifndef AOC_PIN
#define AOC_PIN 1
#endif
#define AOC_PINNED_CONSTS(DIAGONAL)                                      \
    KConst k = kc;                                                       \
    TrigK<real> tk;                                                      \
    if (AOC_PIN) { pin_consts<DIAGONAL>(k); pin_trig(tk); }

// The loop carries a strictly serial chain (x_t -> x_{t+1}), so the only way to keep HBM busy from
// one wavefront is to run the (u, du) loads far ahead: a register ring of ROLL_PF stages.
#ifndef AOC_ROLL_PF
#define AOC_ROLL_PF 8
#endif
constexpr int ROLL_PF = AOC_ROLL_PF;

template <bool DIAG, bool RPT, bool WRITE, typename XO>
__device__ __forceinline__ real rollout(const KConst& k, const real* __restrict__ ref, int tile, int lane,
                                          const real x0[6], const real* __restrict__ u,
                                          const real* __restrict__ du, real a, bool wmask,
                                          XO* __restrict__ x_out, real* __restrict__ u_out, int& flags) {
    const int T = k.T;
    real xs[6], xn[6], q[6], r[2], rb[8];
    real JJ = R(0.0);
#pragma unroll
    for (int c = 0; c < 6; c++) xs[c] = x0[c];
    if (WRITE && wmask) {
#pragma unroll
        for (int c = 0; c < 6; c++) x_out[tix<6>(tile, T, 0, c, lane)] = (XO)xs[c];
    }
    real ub[ROLL_PF][2], db[ROLL_PF][2];
#pragma unroll
    for (int i = 0; i < ROLL_PF; i++) {
        const int t = i < T - 1 ? i : T - 2;
        ub[i][0] = ld_stream3(&u[tix<2>(tile, T, t, 0, lane)]);
        ub[i][1] = ld_stream3(&u[tix<2>(tile, T, t, 1, lane)]);
        db[i][0] = du ? ld_stream3(&du[tix<2>(tile, T, t, 0, lane)]) : R(0.0);
        db[i][1] = du ? ld_stream3(&du[tix<2>(tile, T, t, 1, lane)]) : R(0.0);
    }
    for (int t0 = 0; t0 < T - 1; t0 += ROLL_PF) {
#pragma unroll
        for (int i = 0; i < ROLL_PF; i++) {
            const int t = t0 + i;
            if (t >= T - 1) break;
            const real uc0 = ub[i][0], uc1 = ub[i][1], dc0 = db[i][0], dc1 = db[i][1];
            {   // refill this slot with stage t + ROLL_PF (clamped: the tail re-reads the last stage)
                const int tn = t + ROLL_PF < T - 1 ? t + ROLL_PF : T - 2;
                ub[i][0] = ld_stream3(&u[tix<2>(tile, T, tn, 0, lane)]);
                ub[i][1] = ld_stream3(&u[tix<2>(tile, T, tn, 1, lane)]);
                if (du) {
                    db[i][0] = ld_stream3(&du[tix<2>(tile, T, tn, 0, lane)]);
                    db[i][1] = ld_stream3(&du[tix<2>(tile, T, tn, 1, lane)]);
                }
            }
            real u0, u1;
            step_inputs(uc0, uc1, a, dc0, dc1, u0, u1);
            JJ += stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, t, rb), q, r);
            if (WRITE && !(xs[2] > R(0.0))) flags |= AOC_ST_VNONPOS;  // trials are silent: only the update reports
            const SC s = trig(xs[3], xs[5]);
            step_state(k, xs, u0, u1, s, xn);
            if (WRITE && wmask) {
                st_stream(&u_out[tix<2>(tile, T, t, 0, lane)], u0);
                st_stream(&u_out[tix<2>(tile, T, t, 1, lane)], u1);
#pragma unroll
                for (int c = 0; c < 6; c++) st_stream(&x_out[tix<6>(tile, T, t + 1, c, lane)], (XO)xn[c]);
            }
#pragma unroll
            for (int c = 0; c < 6; c++) xs[c] = xn[c];
        }
    }
    JJ += term_cost2<DIAG>(k, xs, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
    JJ = R(0.5) * JJ;  // JJ accumulated twice the cost, see stage_cost2
    if (WRITE && wmask) {
        u_out[tix<2>(tile, T, T - 1, 0, lane)] = R(0.0);  // optcon.py:193: uu_temp[:, T-1] stays 0
        u_out[tix<2>(tile, T, T - 1, 1, lane)] = R(0.0);
    }
    return JJ;
}

template <bool DIAG, bool RPT, bool WRITE, typename XO>
__global__ __launch_bounds__(TILE) void k_rollout_cost(KConst k, const real* __restrict__ ref,
                                                       const real* __restrict__ x0, const real* __restrict__ u,
                                                       const real* __restrict__ du, const real* __restrict__ alpha,
                                                       XO* __restrict__ x_out, real* __restrict__ u_out,
                                                       real* __restrict__ J_out, int* __restrict__ status) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane;
    real xs[6];
#pragma unroll
    for (int c = 0; c < 6; c++) xs[c] = x0[((size_t)tile * 6 + c) * TILE + lane];
    const real a = (du && alpha) ? alpha[b] : R(0.0);
    int flags = 0;
    const real JJ = rollout<DIAG, RPT, WRITE, XO>(k, ref, tile, lane, xs, u, du, a, true, x_out, u_out, flags);
    if (JJ != JJ || JJ - JJ != R(0.0)) flags |= AOC_ST_NAN;
    J_out[b] = JJ;
    if (status && flags) status[b] |= flags;
}

// Dynamics.get_initial_trajectory (aircraft_simplified.py:126-148): P-controller rollout from x0.
template <bool RPT, typename XO>
__global__ __launch_bounds__(TILE) void k_initial_traj(KConst k, real kp, real kt, const real* __restrict__ ref,
                                                       const real* __restrict__ x0, XO* __restrict__ x_out,
                                                       real* __restrict__ u_out) {
    const int tile = blockIdx.x, lane = threadIdx.x, T = k.T;
    real xs[6], xn[6], rb[8];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        xs[c] = x0[((size_t)tile * 6 + c) * TILE + lane];
        x_out[tix<6>(tile, T, 0, c, lane)] = (XO)xs[c];
    }
    for (int i = 0; i < T - 1; i++) {
        const real* xr = ref_row<RPT>(k, ref, tile, lane, i + 1, rb);
        real u0, u1;
        {
#pragma clang fp contract(off)
            u0 = kp * ((xs[0] - xr[0]) + (xs[1] - xr[1]));  // :143
            u1 = kt * ((xs[3] - xr[3]) + (xs[5] - xr[5]));  // :144
        }
        const SC s = trig(xs[3], xs[5]);
        step_state(k, xs, u0, u1, s, xn);
        u_out[tix<2>(tile, T, i, 0, lane)] = u0;
        u_out[tix<2>(tile, T, i, 1, lane)] = u1;
#pragma unroll
        for (int c = 0; c < 6; c++) { x_out[tix<6>(tile, T, i + 1, c, lane)] = (XO)xn[c]; xs[c] = xn[c]; }
    }
    u_out[tix<2>(tile, T, T - 1, 0, lane)] = R(0.0);
    u_out[tix<2>(tile, T, T - 1, 1, lane)] = R(0.0);
}

