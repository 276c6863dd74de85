// passes/ensemble.inc — closed-loop tracking ensembles about a shared optimum (aoc_track_ensemble).
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// The loop of lqr_tracking.py:279-281 for many members about ONE optimum: u_t = u_opt_t + K_t (x_t - x_opt_t),
// x_{t+1} = step(x_t, u_t) + d_t, in the arithmetic of k_track_rollout.  What k_track_rollout streams per lane and stage
// (x_opt, u_opt, K: 136-160 B) is here one 160-byte record per stage and OPTIMUM,
//     nominal[opt][t][20] = x_opt[0..5], u_opt[0..1], K row 0 [0..5], K row 1 [0..5],
// whose address depends on blockIdx and t only.  It reaches the lanes through LDS: the wavefront loads a block of
// ENS_BLK records cooperatively (ENS_PF coalesced doubles per lane, one block ahead), and every stage reads its record
// back with ten ds_read_b128 at one address for all lanes — a broadcast — one stage ahead of its use.  Scalar loads into
// SGPRs were the first form and are what the compiler makes of a plain uniform access, but a record is 40 SGPRs beside
// the ~100 the model constants, weights and sin/cos coefficients already compete for: the compiler then parks uniform
// values in VGPR lanes (130-180 v_readlane / v_writelane per stage) and waits for the record right behind its load
// (DESIGN.md section 11).  The stats-only instance touches HBM per lane only for x0 and the sixteen statistics.
// Only the fp64 build launches these kernels (there is no float32-arithmetic entry point): the template is never
// instantiated in the float namespace.
// ---------------------------------------------------------------------------------------------
constexpr int ENS_REC = 20;     // doubles per stage record
constexpr int ENS_NSTAT = 16;   // AOC_ENS_NSTAT
constexpr int ENS_BLK = 16;     // stage records per cooperative load
constexpr int ENS_PF = ENS_BLK * ENS_REC / TILE;   // doubles per lane and block
static_assert(ENS_PF * TILE == ENS_BLK * ENS_REC, "a block of records is a whole number of doubles per lane");

// max over |v| with a NaN that sticks (fmax would drop it): for non-negative doubles the IEEE order is the order of
// the bit patterns as unsigned integers, and every NaN lies above +inf there
__device__ __forceinline__ void ens_absmax(unsigned long long& m, double v) {
    const unsigned long long a = (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull;
    m = a > m ? a : m;
}

__device__ __forceinline__ bool ens_finite6(const real x[6]) {
    return __builtin_isfinite(x[0]) && __builtin_isfinite(x[1]) && __builtin_isfinite(x[2]) && __builtin_isfinite(x[3]) &&
           __builtin_isfinite(x[4]) && __builtin_isfinite(x[5]);
}

// WRITE: x_reg / u_reg / dist_out (each may still be NULL) are written; NOISE: d_t drawn by mpc_noise_draw with the counter
// (first + member, step + t, c / 2, 0); the stats-only, noise-free instance carries neither stores nor the generator.
template <bool WRITE, bool NOISE, typename XO, bool DIAG>
__global__ __launch_bounds__(TILE) void k_track_ensemble(KConst kc, int tiles_per_opt, const real* __restrict__ nominal,
                                                         const real* __restrict__ x0, MpcNoise nz, XO* __restrict__ x_reg,
                                                         real* __restrict__ u_reg, real* __restrict__ dist_out,
                                                         real* __restrict__ stats, int* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) real sh[2][ENS_BLK * ENS_REC];
    // uniform constants in VGPRs (aoc_device.h pin_consts) where the SGPRs do not hold them: the diagonal weights (dense
    // ones are re-loaded from the kernel arguments inside the stage), and beside the generator's constants the model too
    KConst k = kc;
    if (DIAG) pin_weights<true>(k);
    if (NOISE) pin_model(k);
    const int tile = blockIdx.x, lane = threadIdx.x, T = k.T;
    const real* __restrict__ nom = nominal + (size_t)(tile / tiles_per_opt) * T * ENS_REC;   // wave-uniform
    int member = tile * TILE + lane;
    if (member >= k.B) member = k.B - 1;   // lanes beyond B replicate member B-1, its draws included
    const size_t nrec = (size_t)T * ENS_REC;
    real xs[6], xn[6], cur[ENS_REC], q[6], r[2], pf[ENS_PF];
    // block b of the nominal = records b*ENS_BLK + 1 .. (b+1)*ENS_BLK (what the stages b*ENS_BLK .. read AHEAD), one
    // coalesced load of ENS_PF doubles per lane; indices beyond the last record are clamped onto it
    auto fetch = [&](int b) {
#pragma unroll
        for (int i = 0; i < ENS_PF; i++) {
            const size_t e = ((size_t)b * ENS_BLK + 1) * ENS_REC + i * TILE + lane;
            pf[i] = nom[e < nrec ? e : nrec - 1];
        }
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int i = 0; i < ENS_PF; i++) sh[b & 1][i * TILE + lane] = pf[i];
        __syncthreads();   // one wavefront: orders the LDS writes before the broadcast reads, costs nothing
    };
    unsigned long long mx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    real JJ = R(0.0);
    int flags = 0, first_bad = T;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        xs[c] = x0[((size_t)tile * 6 + c) * TILE + lane];
        if (WRITE && x_reg) st_stream(&x_reg[tix<6>(tile, T, 0, c, lane)], (XO)xs[c]);
    }
#pragma unroll
    for (int j = 0; j < ENS_REC; j++) cur[j] = nom[j];
    fetch(0);
    stash(0);
    for (int b = 0, t0 = 0; t0 < T - 1; b++, t0 += ENS_BLK) {
      fetch(b + 1);   // in flight during the ENS_BLK stages below
      const int n = T - 1 - t0 < ENS_BLK ? T - 1 - t0 : ENS_BLK;
      for (int i = 0; i < n; i++) {
        const int t = t0 + i;
        real d[6], u0, u1;
        // uu_reg = uu_opt + KK @ (xx_reg - xx_opt)   (lqr_tracking.py:280), summed from 0 in index order
#pragma unroll
        for (int c = 0; c < 6; c++) d[c] = xs[c] - cur[c];
        real a0 = R(0.0), a1 = R(0.0);
#pragma unroll
        for (int c = 0; c < 6; c++) {
            a0 += cur[8 + c] * d[c];
            a1 += cur[14 + c] * d[c];
        }
        u0 = cur[6] + a0;
        u1 = cur[7] + a1;
        const bool vbad = !(xs[2] > R(0.0)), nonfin = !ens_finite6(xs);
        if (vbad) flags |= AOC_ST_VNONPOS;
        if (nonfin) flags |= AOC_ST_NAN;
        if ((vbad || nonfin) && t < first_bad) first_bad = t;
#pragma unroll
        for (int c = 0; c < 6; c++) ens_absmax(mx[c], d[c]);
        ens_absmax(mx[6], u0 - cur[6]);
        ens_absmax(mx[7], u1 - cur[7]);
        JJ += stage_cost2<DIAG>(k, xs, u0, u1, cur, q, r);   // as k_traj_cost with ref = (x_opt, u_opt)
        // Everything that reads the record is above; the plant step below (three quarters of the stage) does not.  The
        // record of stage t+1 is read HERE from LDS — every lane the same address: a broadcast — into the registers this
        // one leaves, and lands behind the step.
        const real* __restrict__ rn = &sh[b & 1][i * ENS_REC];
#pragma unroll
        for (int j = 0; j < ENS_REC; j++) cur[j] = rn[j];
        const SC s = trig(xs[3], xs[5]);
        step_state(k, xs, u0, u1, s, xn);
        if (NOISE) {
            MpcNoise nt = nz;
            nt.step = nz.step + (unsigned)t;
            double dn[6];
            mpc_noise_draw(nt, nz.first + (unsigned)member, dn);
#pragma unroll
            for (int c = 0; c < 6; c++) {
                xn[c] = xn[c] + (real)dn[c];
                if (WRITE && dist_out) st_stream(&dist_out[tix<6>(tile, T, t, c, lane)], (real)dn[c]);
            }
        } else if (WRITE && dist_out) {
#pragma unroll
            for (int c = 0; c < 6; c++) st_stream(&dist_out[tix<6>(tile, T, t, c, lane)], R(0.0));
        }
        if (WRITE && x_reg) {
            st_stream(&u_reg[tix<2>(tile, T, t, 0, lane)], u0);
            st_stream(&u_reg[tix<2>(tile, T, t, 1, lane)], u1);
#pragma unroll
            for (int c = 0; c < 6; c++) st_stream(&x_reg[tix<6>(tile, T, t + 1, c, lane)], (XO)xn[c]);
        }
#pragma unroll
        for (int c = 0; c < 6; c++) xs[c] = xn[c];
      }
      stash(b + 1);
    }
    // sample T-1: deviation, terminal cost, the last look at the domain (no input, no gain: only x_opt of the record is used)
    real dT[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        dT[c] = xs[c] - cur[c];
        ens_absmax(mx[c], dT[c]);
    }
    const bool nonfin = !ens_finite6(xs);
    if (nonfin) flags |= AOC_ST_NAN;
    if ((nonfin || !(xs[2] > R(0.0))) && T - 1 < first_bad) first_bad = T - 1;
    JJ += term_cost2<DIAG>(k, xs, cur, q);
    if (WRITE && x_reg) {
        st_stream(&u_reg[tix<2>(tile, T, T - 1, 0, lane)], R(0.0));
        st_stream(&u_reg[tix<2>(tile, T, T - 1, 1, lane)], R(0.0));
    }
    if (WRITE && dist_out) {
#pragma unroll
        for (int c = 0; c < 6; c++) st_stream(&dist_out[tix<6>(tile, T, T - 1, c, lane)], R(0.0));
    }
    real* __restrict__ so = stats + (size_t)tile * ENS_NSTAT * TILE + lane;
#pragma unroll
    for (int i = 0; i < 8; i++) so[i * TILE] = (real)__longlong_as_double((long long)mx[i]);
    so[8 * TILE] = R(0.5) * JJ;   // JJ accumulated twice the cost, see stage_cost2
#pragma unroll
    for (int c = 0; c < 6; c++) so[(9 + c) * TILE] = dT[c];
    so[15 * TILE] = (real)first_bad;
    if (status && flags) status[tile * TILE + lane] |= flags;
}

#ifndef AOC_KERNELS_ONLY
// Body of aoc_track_ensemble.  A template only so that the kernels it names are instantiated where it is called — from
// the fp64 entry point — and not once more in the float32 namespace.
template <typename = void>
static int api_track_ensemble(const aoc_problem* p, int32_t n_opt, int32_t members_per_opt, const real* nominal,
                              const real* x0_reg, const aoc_mpc_noise* noise, void* x_reg, real* u_reg, real* dist_out,
                              real* stats, int32_t* status) {
    if (!p) return einval("aoc_track_ensemble: aoc_problem is NULL");
    if (!nominal) return einval("aoc_track_ensemble: nominal is NULL");
    if (!x0_reg) return einval("aoc_track_ensemble: x0_reg is NULL");
    if (!stats) return einval("aoc_track_ensemble: stats is NULL");
    if (n_opt < 1) return einval("aoc_track_ensemble: n_opt = %d (need n_opt >= 1)", n_opt);
    if (members_per_opt < TILE || members_per_opt % TILE)
        return einval("aoc_track_ensemble: members_per_opt = %d is not a positive multiple of %d", members_per_opt, TILE);
    if (p->T < 3) return einval("aoc_track_ensemble: T = %d (need T >= 3)", p->T);
    if ((long long)p->B <= (long long)(n_opt - 1) * members_per_opt || (long long)p->B > (long long)n_opt * members_per_opt)
        return einval("aoc_track_ensemble: B = %d members do not fill n_opt = %d groups of members_per_opt = %d (need %lld < B <= %lld)",
                      p->B, n_opt, members_per_opt, (long long)(n_opt - 1) * members_per_opt, (long long)n_opt * members_per_opt);
    if ((x_reg == nullptr) != (u_reg == nullptr))
        return einval("aoc_track_ensemble: x_reg and u_reg go together (one of them is NULL)");
    if (p->x_out_f32 && x_reg && noise)
        return einval("aoc_track_ensemble: float32 state storage (x_out_f32 = 1) cannot hold disturbed states: with noise "
                      "x_reg must be fp64");
    if (p->RRt[1] != p->RRt[2])
        return einval("aoc_track_ensemble: aoc_problem.RRt is not symmetric (R01 = %g, R10 = %g)", p->RRt[1], p->RRt[2]);
    KConst k = make_const(p->model, p->QQt, p->RRt, p->QQT, p->B, p->T);
    MpcNoise nz;
    memset(&nz, 0, sizeof nz);
    if (noise) {
        nz.key0 = (unsigned)(noise->seed & 0xffffffffull); nz.key1 = (unsigned)(noise->seed >> 32);
        nz.step = noise->step; nz.first = noise->first;
        for (int c = 0; c < 6; c++) nz.sigma[c] = noise->sigma[c];
        nz.on = 1;
    }
    hipStream_t st = (hipStream_t)p->stream;
    const int tpo = members_per_opt / TILE;
    const bool write = x_reg || dist_out;
#define AOC_ENS_LAUNCH(W, N, XO, D)                                                                                     \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo, nominal, x0_reg, nz, \
                       (XO*)x_reg, u_reg, dist_out, stats, status)
    if (p->x_out_f32 && x_reg)   // (never with noise, see above)
        AOC_DISPATCH_BOOL(k.diag, D, AOC_ENS_LAUNCH(true, false, float, D));
    else
        AOC_DISPATCH_BOOL(write, W, AOC_DISPATCH_BOOL(nz.on, N, AOC_DISPATCH_BOOL(k.diag, D, AOC_ENS_LAUNCH(W, N, double, D))));
#undef AOC_ENS_LAUNCH
    return check_launch("aoc_track_ensemble");
}
#endif  // AOC_KERNELS_ONLY

