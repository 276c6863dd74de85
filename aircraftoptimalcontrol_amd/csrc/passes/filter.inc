// passes/filter.inc — the gains of the Kalman filter linearised about each optimum, on the device (aoc_filter_gains).
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// The filter Riccati recursion for the measurement y = H dx + v, H a selection of channels (the 6-bit mask `measured`),
// V = diag(rho^2), W = diag(sigma^2), P^-_0 = Sigma0, A_t the Jacobian of the plant step at (x_opt_t, u_opt_t) — A, not
// F = A + B K: the filter knows its input.  The measurement update takes one SCALAR measurement at a time: Q = P^-_t, then for
// c = 0 .. 5 in this order, where bit c of `measured` is set, with v_c = rho[c]^2 and s = 1 / (Q_cc + v_c),
//     row and column c:      Q_ic <- Q_ic (v_c s)            multiplicative: no subtraction, so no cancellation
//     every other entry:     Q_ij <- Q_ij - (Q_ic Q_cj) s
// and after the sixth channel P^+_t = Q, L_t[:, c] = P^+_t[:, c] / v_c (exactly +0.0 for an unmeasured c), and for t <= T-2
// P^-_{t+1} = A_t P^+_t A_t^T + W.  No matrix inverse, no pivoting.
//
// Two kernels, as in covariance.inc:
//   k_cov_stage<false>  the stage kernel of covariance.inc without the B K term: A_t in the same COV_REC-double record.
//   k_filter_chain      one wavefront per optimum, serial in t, lane 6i+j the entry (i,j) of Q (lanes 36-63 own nothing).
//                       The time update is k_cov_chain's two rounds with A in place of F — the same dot6 / row6 on the same
//                       operands, so with measured = 0 the P^- records are the covariance call's bits with zero gains.
//                       A downdate needs row c of Q in every lane: by symmetry lane (i,j) needs Q_ci, Q_cj and the pivot
//                       Q_cc.  They come by cross-lane moves from the lanes (c,i), (c,j) and (c,c): two ds_bpermute_b32 per
//                       operand, v_readlane for the pivot, no LDS write and no barrier on the chain.  (Through LDS — the
//                       six lanes of row c write, a barrier, all lanes read their three — was built first and is 4 %
//                       slower: 0.964 against 0.925 ms for one optimum and T = 1000, 1.384 against 1.364 ms for 1024
//                       optima; EXPERIMENTS.md.)  The lanes (i,j) and (j,i) evaluate the same expression on the same operands
//                       (a product commutes), so Q stays symmetric bit for bit.  s is a true fp64 division.
//                       P^-_t and P^+_t of a sample stay in LDS until the next stage has started; L_t (36 doubles, lanes
//                       0-35, coalesced) and the covariance record (FILT_NREC = 42 doubles: the upper triangles of P^-_t and
//                       P^+_t row by row, lanes 0-41) are gathered from there one stage later, off the chain.  The division
//                       by v_c of L is Markstein's three-instruction form with RN(1 / v_c) from the host: correctly rounded.
// No atomics, no private scratch; an optimum's bits depend on nothing but its own inputs.
// Only the fp64 build launches these kernels: the templates are never instantiated in the float namespace.
// ---------------------------------------------------------------------------------------------
constexpr int FILT_NREC = 42;   // AOC_FILT_NREC

struct FiltV { double v[6], rv[6]; int measured; };   // rho^2, RN(1 / rho^2) (measured channels; 1 elsewhere), the mask

// LDS of k_filter_chain beside the stream's double buffer: st[2][72] = P^- [36] and P^+ [36] of even / odd samples, y[64] the
// results of round 1.
constexpr int FILT_PP = 36, FILT_ST = 72, FILT_Y = 2 * FILT_ST, FILT_LDS = FILT_Y + TILE;
static_assert(FILT_PP % 2 == 0 && FILT_ST % 2 == 0 && FILT_Y % 2 == 0, "rows of P^+ and of y start on 16 bytes");

template <typename = void>
__global__ __launch_bounds__(TILE) void k_filter_chain(int T, const real* __restrict__ rec, const real* __restrict__ Sigma0,
                                                       CovW W, FiltV V, real* __restrict__ filter, real* __restrict__ cov,
                                                       int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real sh[2][COV_BLK * COV_REC];
    __shared__ __attribute__((aligned(16))) real ws[FILT_LDS];
    const int opt = blockIdx.x, L = threadIdx.x;
    const real* __restrict__ rc = rec + (size_t)opt * T * COV_REC;   // wave-uniform
    const size_t nrec = (size_t)T * COV_REC;
    // ---- what this lane computes (fixed for the whole kernel) ----
    const bool isP = L < 36;
    const int pi = isP ? L / 6 : 0, pj = isP ? L % 6 : 0, pa = pi < pj ? pi : pj, pb = pi < pj ? pj : pi;
    const real w = (isP && pi == pj) ? (real)W.w[pi] : R(0.0);
    const bool lcol = ((V.measured >> pj) & 1) != 0;                 // column j of L is a measured channel's
    const real vj = (real)V.v[pj], rvj = (real)V.rv[pj];
    // the covariance record's entry this lane stores (lanes 0-41): the upper triangles of P^- and of P^+
    int src = 0;
    if (L < FILT_NREC) {
        int e = L < 21 ? L : L - 21, i = 0;
        while (e >= 6 - i) { e -= 6 - i; i++; }
        src = (L < 21 ? 0 : FILT_PP) + i * 6 + i + e;
    }

    real pf[COV_PF];
    auto fetch = [&](int b) { cov_fetch(rc, nrec, b, L, pf); };
    auto stash = [&](int b) { cov_stash(sh[b & 1], L, pf); };
    int flags = 0;
    real q = R(0.0);   // this lane's entry of Q
    // The measurement update of sample t on q (= P^-_t, which is in LDS already); leaves P^+_t in q and in LDS.
    auto measure = [&](int t) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
            if (!((V.measured >> c) & 1)) continue;                  // wave-uniform
            const real qi = __shfl(q, c * 6 + pi), qj = __shfl(q, c * 6 + pj);
            const real d = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(q), 7 * c),
                                            __builtin_amdgcn_readlane(__double2loint(q), 7 * c)) + (real)V.v[c];
            const real s = div_r(R(1.0), d);
            if (!(d > R(0.0))) flags |= AOC_ST_SINGULAR;
            q = (pi == c || pj == c) ? q * ((real)V.v[c] * s) : fma_r(-(qi * qj), s, q);
        }
        if (isP) ws[(t & 1) * FILT_ST + FILT_PP + L] = q;
        __syncthreads();
    };
    // L_t and the covariance record of sample t_out go out
    auto emit = [&](int t_out) {
        const real* __restrict__ st = &ws[(t_out & 1) * FILT_ST];
        if (isP) filter[((size_t)opt * T + t_out) * 36 + L] = lcol ? div_by_const(st[FILT_PP + L], vj, rvj) : R(0.0);
        if (cov && L < FILT_NREC) cov[((size_t)opt * T + t_out) * FILT_NREC + L] = st[src];
    };

    // ---- sample 0 ----
    if (isP && Sigma0) q = Sigma0[(size_t)opt * 21 + sidx(pa, pb)];
    if (isP) ws[L] = q;
    fetch(0);
    stash(0);
    for (int b = 0, t0 = 0; t0 < T - 1; b++, t0 += COV_BLK) {
      fetch(b + 1);   // in flight during the COV_BLK stages below
      const int n = T - 1 - t0 < COV_BLK ? T - 1 - t0 : COV_BLK;
      for (int i = 0; i < n; i++) {
        const int t = t0 + i;
        const real* __restrict__ rn = &sh[b & 1][i * COV_REC];
        real a1[6], b2[6], x1[6], x2[6];
        row6(rn + pi * 6, a1);        // the stream: nothing here waits for the previous stage
        row6(rn + pb * 6, b2);
        flags |= (int)rn[COV_O_FLAG];
        measure(t);                   // P^+_t is in LDS
        row6(&ws[(t & 1) * FILT_ST + FILT_PP + pj * 6], x1);   // column j of P^+ as its row j
        if (t > 0) emit(t - 1);
        const real y = dot6(a1, x1, R(0.0));
        ws[FILT_Y + L] = y;
        __syncthreads();              // (and sample t - 1 is read before its slots are written again below)
        row6(&ws[FILT_Y + pa * 6], x2);
        q = dot6(x2, b2, w);
        if (isP) ws[((t + 1) & 1) * FILT_ST + L] = q;
      }
      stash(b + 1);
    }
    flags |= (int)sh[((T - 1) / COV_BLK) & 1][((T - 1) % COV_BLK) * COV_REC + COV_O_FLAG];
    measure(T - 1);
    emit(T - 2);
    emit(T - 1);
    if (L == 0 && status && flags) status[opt] |= flags;
}

#ifndef AOC_KERNELS_ONLY
// aoc_filter_gains_scratch_bytes: the records of k_cov_stage, [n_opt][T][COV_REC]; 0 for a geometry the call refuses anyway
static size_t filter_gains_scratch_bytes(int32_t n_opt, int32_t T) { return track_covariance_scratch_bytes(n_opt, T); }

// Body of aoc_filter_gains.  A template only so that the kernels it names are instantiated where it is called — from the
// fp64 entry point — and not once more in the float32 namespace.
template <typename = void>
static int api_filter_gains(const aoc_problem* p, int32_t n_opt, const real* nominal, const real* Sigma0,
                            const aoc_mpc_noise* noise, const double* rho, int32_t measured, real* filter, real* cov,
                            int32_t* status, void* scratch, size_t scratch_bytes) {
    const char* fn = "aoc_filter_gains";
    if (!p) return einval("%s: aoc_problem is NULL", fn);
    if (!nominal) return einval("%s: nominal is NULL", fn);
    if (!filter) return einval("%s: filter is NULL", fn);
    if (!rho) return einval("%s: rho is NULL", fn);
    if (n_opt < 1) return einval("%s: n_opt = %d (need n_opt >= 1)", fn, n_opt);
    if (p->T < 3) return einval("%s: T = %d (need T >= 3)", fn, p->T);
    if (measured < 0 || measured > 63) return einval("%s: measured = %d (a mask of the six channels: 0 .. 63)", fn, measured);
    FiltV V;
    V.measured = measured;
    for (int c = 0; c < 6; c++) {
        V.v[c] = V.rv[c] = 1.0;   // (the rho of an unmeasured channel is not read)
        if (!((measured >> c) & 1)) continue;
        if (!(rho[c] > 0.0) || !__builtin_isfinite(rho[c]))
            return einval("%s: rho[%d] = %g (a measured channel needs a finite rho > 0)", fn, c, rho[c]);
        V.v[c] = rho[c] * rho[c];
        V.rv[c] = 1.0 / V.v[c];
    }
    CovW W;
    for (int c = 0; c < 6; c++) {
        const double s = noise ? noise->sigma[c] : 0.0;
        if (!(s >= 0.0) || !__builtin_isfinite(s)) return einval("%s: sigma[%d] = %g (need a finite sigma >= 0)", fn, c, s);
        W.w[c] = s * s;
    }
    const size_t need = filter_gains_scratch_bytes(n_opt, p->T);
    if (!scratch) return einval("%s: scratch is NULL (need %zu bytes, aoc_filter_gains_scratch_bytes)", fn, need);
    if ((uintptr_t)scratch % 16) return einval("%s: scratch must be 16-byte aligned", fn);
    if (scratch_bytes < need)
        return einval("%s: scratch_bytes = %zu, need %zu (aoc_filter_gains_scratch_bytes)", fn, scratch_bytes, need);
    KConst k = make_const(p->model, nullptr, nullptr, nullptr, n_opt, p->T);
    hipStream_t st = (hipStream_t)p->stream;
    const size_t total = (size_t)n_opt * p->T;
    hipLaunchKernelGGL(k_cov_stage<false>, dim3((unsigned)((total + COV_THREADS - 1) / COV_THREADS)), dim3(COV_THREADS), 0, st,
                       k, n_opt, nominal, (real*)scratch);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(k_filter_chain<>, dim3(n_opt), dim3(TILE), 0, st, p->T, (const real*)scratch, Sigma0, W, V, filter, cov,
                       status);
    return check_launch(fn);
}
#endif  // AOC_KERNELS_ONLY
