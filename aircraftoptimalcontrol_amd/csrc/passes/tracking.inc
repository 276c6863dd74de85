// passes/tracking.inc — lqr_tracking: tracking gains and the closed-loop rollout.
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// LQR tracking (lqr_tracking.py:245-283): linearise about (x_opt,u_opt), non-augmented Riccati with
// constant weights and S = 0, gains K (2x6), closed-loop nonlinear rollout.
// ---------------------------------------------------------------------------------------------

// a run-time zero: every gain kernel then compiles the same arithmetic for the affine terms (the tracking problem has
// q = r = 0, S = 0)
__device__ __forceinline__ real track_zero() {
    real zz = R(0.0);
    bw_opaque(zz);
    return zz;
}
// One stage of the tracking gains, whichever kernel runs it: the Riccati stage on (P, p) with the run-time zero for the
// affine terms, the gain columns 1..6 stored into Kout at sample t (no feed-forward column here); the status bits back.
__device__ __forceinline__ int track_gain_stage(const KConst& k, const Lin& l, real P[21], real p[6], const real Qb[21],
                                                real* __restrict__ Kout, int tile, int T, int t, int lane) {
    const real zz = track_zero();
    const real z6[6] = {zz, zz, zz, zz, zz, zz}, z2[2] = {zz, zz};
    const StageFlags fl = lqr_stage(k, l, P, p, Qb, zz, zz, zz, z6, z2, [&](int c, real a, real b) {
        if (c >= 1) {
            Kout[tix<12>(tile, T, t, c - 1, lane)] = a;
            Kout[tix<12>(tile, T, t, 5 + c, lane)] = b;
        }
    });
    int flags = 0;
    if (fl.singular) flags |= AOC_ST_SINGULAR;
    if (fl.regularised) flags |= AOC_ST_REGULARISED;
    return flags;
}

template <bool DIAG, typename XT>
__global__ __launch_bounds__(TILE) void k_track_gains(KConst k, const XT* __restrict__ x,
                                                      const real* __restrict__ u, const real* __restrict__ x_opt0,
                                                      real* __restrict__ Kout, int* __restrict__ status) {
    const int tile = blockIdx.x, lane = threadIdx.x, T = k.T;
    real P[21], p[6], Qb[21], xs[6], xn[6];
    int flags = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        p[i] = R(0.0);
#pragma unroll
        for (int j = i; j < 6; j++) { P[sidx(i, j)] = k.QT[i * 6 + j]; Qb[sidx(i, j)] = k.Q[i * 6 + j]; }  // :716
    }
    load_state(x, x_opt0, tile, T, T - 2, lane, xn);
    real un0 = u[tix<2>(tile, T, T - 2, 0, lane)];
    for (int t = T - 2; t >= 0; t--) {
#pragma unroll
        for (int c = 0; c < 6; c++) xs[c] = xn[c];
        const real u0 = un0;
        if (t > 0) {
            load_state(x, x_opt0, tile, T, t - 1, lane, xn);
            un0 = u[tix<2>(tile, T, t - 1, 0, lane)];
        }
        const SC s = trig(xs[3], xs[5]);
        Lin l = linearise(k, xs, u0, s);
        track_lin_fields(l, [](int, real& v) { bw_opaque(v); });   // same cut as k_track_gains2, same roundings
        flags |= track_gain_stage(k, l, P, p, Qb, Kout, tile, T, t, lane);
    }
#pragma unroll
    for (int j = 0; j < 12; j++) Kout[tix<12>(tile, T, T - 1, j, lane)] = R(0.0);  // KK[:,:,T-1] stays 0 (:700)
    if (status && flags) status[tile * TILE + lane] |= flags;
}

// Small batches: linearisation (wavefront 0, one stage ahead) and Riccati/gain recursion (wavefront 1), as k_backward2.
template <bool DIAG, typename XT>
__global__ __launch_bounds__(2 * TILE) void k_track_gains2(KConst kc, const XT* __restrict__ x,
                                                           const real* __restrict__ u, const real* __restrict__ x_opt0,
                                                           real* __restrict__ Kout, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real sh[2][6][TILE][2];   // two fields per lane side by side, see k_backward2
    AOC_PINNED_CONSTS(DIAG)
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), T = k.T;
    const bool producer = threadIdx.x < TILE;
    real P[21], p[6], Qb[21], xs[6];
    int flags = 0;
    XT xb[BWS_PF][6];   // the producer's (x, u0) loads of the next BWS_PF stages, see k_backward2
    real ub[BWS_PF], x0s[6];
    if (producer) {
        load_x0(x_opt0, tile, lane, x0s);
#pragma unroll
        for (int i = 0; i < BWS_PF; i++) {
            const int ts = T - 2 - i > 0 ? T - 2 - i : 0;
#pragma unroll
            for (int c = 0; c < 6; c++) xb[i][c] = x[tix<6>(tile, T, ts, c, lane)];
            ub[i] = u[tix<2>(tile, T, ts, 0, lane)];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            p[i] = R(0.0);
#pragma unroll
            for (int j = i; j < 6; j++) { P[sidx(i, j)] = k.QT[i * 6 + j]; Qb[sidx(i, j)] = k.Q[i * 6 + j]; }  // :716
        }
    }
    // each role runs its own loop, see k_backward2
    if (producer) {
        for (int j0 = 0; j0 < T; j0 += BWS_PF) {   // stage T-2-j
#pragma unroll
          for (int i_ = 0; i_ < BWS_PF; i_++) {
            const int j = j0 + i_;
            if (j >= T) break;
            const int tp = T - 2 - j;
            if (tp >= 0) {
#pragma unroll
                for (int c = 0; c < 6; c++) xs[c] = tp == 0 ? x0s[c] : (real)xb[i_][c];
                const real u0 = ring_take(ub[i_]);
                {
                    const int tn = tp - BWS_PF > 0 ? tp - BWS_PF : 0;
#pragma unroll
                    for (int c = 0; c < 6; c++) xb[i_][c] = x[tix<6>(tile, T, tn, c, lane)];
                    ub[i_] = u[tix<2>(tile, T, tn, 0, lane)];
                }
                const SC s = trig(xs[3], xs[5], tk);
                Lin l = linearise(k, xs, u0, s);
                real(*dst)[TILE][2] = sh[j & 1];
                track_lin_fields(l, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            }
            __syncthreads();
          }
        }
    } else {
        for (int j = 0; j < T; j++) {   // stage T-1-j
          const int tc = T - 1 - j;
          if (j >= 1) {
            Lin l;
            real(*src)[TILE][2] = sh[(j - 1) & 1];
            track_lin_fields(l, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
            flags |= track_gain_stage(k, l, P, p, Qb, Kout, tile, T, tc, lane);
          }
          __syncthreads();
        }
    }
    if (!producer) {
#pragma unroll
        for (int c = 0; c < 12; c++) Kout[tix<12>(tile, T, T - 1, c, lane)] = R(0.0);  // KK[:,:,T-1] stays 0 (:700)
        if (status && flags) atomicOr(&status[tile * TILE + lane], flags);
    }
}

// Tiny batches: one producer and the three column consumers of k_backward4 (no affine terms here: the tracking problem
// has q = r = 0, and no column of P or K depends on them), constants pinned, 16-byte LDS hand-offs.
template <bool DIAG, typename XT>
__global__ __launch_bounds__(4 * TILE) void k_track_gains4(KConst kc, const XT* __restrict__ x,
                                                           const real* __restrict__ u, const real* __restrict__ x_opt0,
                                                           real* __restrict__ Kout, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real sh[2][6][TILE][2];
    __shared__ __attribute__((aligned(16))) real shP[2][11][TILE][2];
    AOC_PINNED_CONSTS(DIAG)
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, T = k.T;
    const bool producer = wv == 0;
    real P[21], p[6], Qb[21], xs[6];
    int flags = 0;
    XT xb[BWS_PF][6];
    real ub[BWS_PF], x0s[6];
    if (producer) {
        load_x0(x_opt0, tile, lane, x0s);
#pragma unroll
        for (int i = 0; i < BWS_PF; i++) {
            const int ts = T - 2 - i > 0 ? T - 2 - i : 0;
#pragma unroll
            for (int c = 0; c < 6; c++) xb[i][c] = x[tix<6>(tile, T, ts, c, lane)];
            ub[i] = u[tix<2>(tile, T, ts, 0, lane)];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            p[i] = R(0.0);
#pragma unroll
            for (int j = i; j < 6; j++) { P[sidx(i, j)] = k.QT[i * 6 + j]; Qb[sidx(i, j)] = k.Q[i * 6 + j]; }  // :716
        }
    }
    // each role runs its own loop, see k_backward2
    if (producer) {
        for (int j0 = 0; j0 < T; j0 += BWS_PF) {   // stage T-2-j
#pragma unroll
          for (int i_ = 0; i_ < BWS_PF; i_++) {
            const int j = j0 + i_;
            if (j >= T) break;
            const int tp = T - 2 - j;
            if (tp >= 0) {
#pragma unroll
                for (int c = 0; c < 6; c++) xs[c] = tp == 0 ? x0s[c] : (real)xb[i_][c];
                const real u0 = ring_take(ub[i_]);
                {
                    const int tn = tp - BWS_PF > 0 ? tp - BWS_PF : 0;
#pragma unroll
                    for (int c = 0; c < 6; c++) xb[i_][c] = x[tix<6>(tile, T, tn, c, lane)];
                    ub[i_] = u[tix<2>(tile, T, tn, 0, lane)];
                }
                const SC s = trig(xs[3], xs[5], tk);
                Lin l = linearise(k, xs, u0, s);
                real(*dst)[TILE][2] = sh[j & 1];
                track_lin_fields(l, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            }
            __syncthreads();
          }
        }
    } else {
        for (int j = 0; j < T; j++) {   // stage T-1-j
          const int tc = T - 1 - j;
          if (j >= 1) {
            const int w3 = wv - 1;
            Lin l;
            real(*src)[TILE][2] = sh[(j - 1) & 1];
            real(*srcP)[TILE][2] = shP[(j - 1) & 1];
            real(*dstP)[TILE][2] = shP[j & 1];
            track_lin_fields(l, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
            const real zz = track_zero();   // the same arithmetic in every gain kernel
            const real z6[6] = {zz, zz, zz, zz, zz, zz}, z2[2] = {zz, zz};
            real Pn[21];
            StageFlags fl;
#define TG4_PART(W, COLS)                                                                        \
            if (w3 == W) {                                                                       \
                if (j >= 2) {                                                                    \
                    _Pragma("unroll") for (int cc = 0; cc < 6; cc++) {                           \
                        if ((COLS >> cc) & 1) continue;                                          \
                        _Pragma("unroll") for (int i = 0; i <= cc; i++) {                        \
                            const int e = cc * (cc + 1) / 2 + i;                                 \
                            P[sidx(i, cc)] = srcP[e >> 1][lane][e & 1];                          \
                        }                                                                        \
                    }                                                                            \
                }                                                                                \
                fl = lqr_stage_part<COLS, false>(k, l, P, p, Qb, zz, zz, zz, z6, z2, Pn,          \
                                                 [&](int c, real a, real b) {                    \
                    Kout[tix<12>(tile, T, tc, c - 1, lane)] = a;                                 \
                    Kout[tix<12>(tile, T, tc, 5 + c, lane)] = b;                                 \
                });                                                                              \
                _Pragma("unroll") for (int cc = 0; cc < 6; cc++) {                               \
                    if (!((COLS >> cc) & 1)) continue;                                           \
                    _Pragma("unroll") for (int i = 0; i <= cc; i++) {                            \
                        const int e = cc * (cc + 1) / 2 + i;                                     \
                        P[sidx(i, cc)] = Pn[sidx(i, cc)];                                        \
                        dstP[e >> 1][lane][e & 1] = Pn[sidx(i, cc)];                             \
                    }                                                                            \
                }                                                                                \
            }
            TG4_PART(0, BW4_C0)
            TG4_PART(1, BW4_C1)
            TG4_PART(2, BW4_C2)
#undef TG4_PART
            if (w3 == 0) {
                if (fl.singular) flags |= AOC_ST_SINGULAR;
                if (fl.regularised) flags |= AOC_ST_REGULARISED;
            }
          }
          __syncthreads();
        }
    }
    if (wv == 1) {
#pragma unroll
        for (int c = 0; c < 12; c++) Kout[tix<12>(tile, T, T - 1, c, lane)] = R(0.0);  // KK[:,:,T-1] stays 0 (:700)
        if (status && flags) atomicOr(&status[tile * TILE + lane], flags);
    }
}

