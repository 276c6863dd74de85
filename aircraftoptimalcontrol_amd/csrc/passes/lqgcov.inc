// passes/lqgcov.inc — joint (dx, e) covariance prediction for the LQG loop of lqg.inc (aoc_track_covariance_lqg).
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// What linear theory predicts for the loop of aoc_track_ensemble_lqg about one optimum, in the coordinates (dx, e) with
// e_t = dx_t - e^+_t the posterior estimation error: A_t, F_t = A_t + B_t K_t, c_t as in covariance.inc, N_t = F_t - A_t,
// J_t = I - L_t, V = diag(rho^2), W = diag(sigma^2); the means m = E dx, mu = E e and the covariances X = cov(dx), E = cov(e),
// C = cov(dx, e) (not symmetric) follow
//     measurement, t = 0 .. T-1:   mu = J mu^-,   E = J E^- J^T + L V L^T,   C = C^- J^T                      (Joseph form: any L)
//     time, t <= T-2:              m' = F m - N mu + c,   mu^-' = A mu,
//                                  Y1 = F X - N C^T,  Y2 = F C - N E,  Y3 = A E,
//                                  X' = Y1 F^T - Y2 N^T + W,   C^-' = Y2 A^T + W,   E^-' = Y3 A^T + W
// from m_0 = mean0, mu^-_0 = mean0 - ehat0, X_0 = C^-_0 = E^-_0 = Sigma0.  The record of one (optimum, sample), LQC_NREC =
// AOC_LQGCOV_NREC = 96 doubles: m [6], mu [6], the upper triangles of X and of E row by row [21 + 21], C row-major [36], the
// mean of du = K (m - mu) [2], its covariance K (X - C - C^T + E) K^T (00, 01, 11) [3], +0.0.
//
// No stage kernel of its own: k_cov_stage<true> (F_t, c_t, K_t) and k_cov_stage<false> (A_t) of covariance.inc, as they are,
// into the two halves of the scratch.
//   k_lqgcov_chain  one wavefront per optimum, serial in t, lane 6i+j owns the entry (i,j) of X, of C and of E; the means and
//                   the input moments ride on the lanes 36-61.  A stage is four dependent rounds of 6-term products, each
//                   through LDS as in k_cov_chain (state rows come back as three ds_read_b128):
//                     lane      A (measure 1)          B (measure 2)          C (time 1)                      D (time 2)
//                     6i+j      G = J_i. E^-_.j        E = G_a. J_b. + LVL_ab Y1, Y2, Y3 (five products)      X', C^-', E^-' (four)
//                               C = C^-_i. J_j.
//                     36+i      mu_i = J_i. mu^-       -                      m'_i = F_i. m - N_i. mu + c_i   -
//                     42+i      -                      -                      mu^-'_i = A_i. mu               -
//                     48+r      -                      -                      K_r. m - K_r. mu                -
//                     50+6r+j   -                      -                      (K H)_rj, H = X - C - C^T + E   -
//                     36+q      -                      -                      -                               (K H)_r. K_s.
//                   (a = min(i,j), b = max(i,j): both halves of X and of E are ONE expression, so they stay symmetric bit for
//                   bit.)  Every lane runs the same five products of round C on operands of its own — K H is Y1 - Y2 with K_r
//                   in place of F_i and of N_i — so the wavefront never diverges on the chain.  C is kept twice, row-major
//                   and transposed, so that its columns come back as rows.  L V L^T does not depend on the chain and is
//                   formed from the stream before round A.  The records of both k_cov_stage instances and L_t are pure
//                   streams, fetched a block of COV_BLK samples ahead into an LDS double buffer.  Everything a record holds
//                   lies in LDS under the parity of its sample until the next stage has started; it leaves as two coalesced
//                   stores (64 + 32 lanes), off the chain.
// Every sum starts from +0.0 and is a chain of fused multiply-adds, differences are taken between such sums: with Sigma0 = 0,
// W = 0 and V = 0 every covariance entry is exactly +0.0 wherever the records are finite.  No atomics, no private scratch; an
// optimum's bits depend on nothing but its own inputs.
// Only the fp64 build launches this kernel: the template is never instantiated in the float namespace.
// ---------------------------------------------------------------------------------------------
constexpr int LQC_NREC = 96;                          // AOC_LQGCOV_NREC
constexpr int LQC_LREC = 36;                          // doubles per sample of `filter`
constexpr int LQC_LPF = COV_BLK * LQC_LREC / TILE;    // doubles of L per lane and block
static_assert(LQC_LPF * TILE == COV_BLK * LQC_LREC, "a block of gains is a whole number of doubles per lane");
// Of k_cov_stage<false>'s record only A_t and the status bits are kept in LDS (c_t and K_t are those of the other record): with
// 56 doubles per sample the kernel's LDS is 44288 bytes, three workgroups per compute unit; with 38 it is 39712, four.
constexpr int LQC_AREC = 38, LQC_A_FLAG = 36;
static_assert(LQC_AREC % 2 == 0, "rows of A start on 16 bytes");

// LDS beside the streams' double buffers, once per parity of the sample (LQC_ST doubles): the state and everything derived
// from it that a later round or the record reads.
constexpr int LQC_X = 0, LQC_CM = 36, LQC_EM = 72, LQC_M = 108, LQC_MUM = 114, LQC_C = 120, LQC_CT = 156, LQC_E = 192,
              LQC_MU = 228, LQC_G = 234, LQC_Y1 = 270, LQC_Y2 = 306, LQC_Y3 = 342, LQC_KH = 378, LQC_O = 390, LQC_ZERO = 396,
              LQC_DUMP = 398, LQC_ST = 400;
static_assert(LQC_M % 2 == 0 && LQC_MUM % 2 == 0 && LQC_MU % 2 == 0 && LQC_G % 2 == 0 && LQC_KH % 2 == 0 && LQC_ST % 2 == 0,
              "rows start on 16 bytes");

template <typename = void>
__global__ __launch_bounds__(TILE) void k_lqgcov_chain(int T, const real* __restrict__ recF, const real* __restrict__ recA,
                                                       const real* __restrict__ filter, const real* __restrict__ mean0,
                                                       const real* __restrict__ ehat0, const real* __restrict__ Sigma0,
                                                       CovW W, CovW V, real* __restrict__ pred, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real shF[2][COV_BLK * COV_REC];
    __shared__ __attribute__((aligned(16))) real shA[2][COV_BLK * LQC_AREC + 2];   // (+ a slot for what is not kept)
    __shared__ __attribute__((aligned(16))) real shL[2][COV_BLK * LQC_LREC];
    __shared__ __attribute__((aligned(16))) real ws[2 * LQC_ST];
    const int opt = blockIdx.x, L = threadIdx.x;
    const real* __restrict__ rcF = recF + (size_t)opt * T * COV_REC;   // wave-uniform
    const real* __restrict__ rcA = recA + (size_t)opt * T * COV_REC;
    const real* __restrict__ rcL = filter + (size_t)opt * T * LQC_LREC;
    const size_t nrec = (size_t)T * COV_REC, nl = (size_t)T * LQC_LREC;
    // ---- what this lane computes (fixed for the whole kernel) ----
    const bool isP = L < 36, isM = L >= 36 && L < 42, isMu = L >= 42 && L < 48, isDu = L >= 48 && L < 50,
               isKH = L >= 50 && L < 62, isQ = L >= 36 && L < 39;
    const int pi = isP ? L / 6 : (isM ? L - 36 : (isMu ? L - 42 : 0)), pj = isP ? L % 6 : (isKH ? (L - 50) % 6 : 0);
    const int pa = pi < pj ? pi : pj, pb = pi < pj ? pj : pi;
    const int kr = isDu ? L - 48 : (isKH ? (L - 50) / 6 : 0);
    const int qr = L == 38 ? 1 : 0, qs = L == 36 ? 0 : 1;
    const bool useK = isDu || isKH;
    // round A: rows of the prior state (E^- row j, or mu^-; C^- row i)
    const int sA1 = isP ? LQC_EM + pj * 6 : LQC_MUM, sA2 = isP ? LQC_CM + pi * 6 : LQC_MUM;
    const int dA1 = isP ? LQC_G + L : (isM ? LQC_MU + pi : LQC_DUMP);
    const int dA2 = isP ? LQC_C + L : LQC_DUMP, dA3 = isP ? LQC_CT + pj * 6 + pi : LQC_DUMP;
    // round B
    const int sB = LQC_G + pa * 6, dB = isP ? LQC_E + L : LQC_DUMP;
    // round C: the left rows f (F_i or K_r) and a (A_i), n = f - a (N_i) or f (K_r); four rows of the posterior state
    const int oF1 = useK ? COV_O_K + kr * 6 : pi * 6, oA1 = pi * 6;
    const int cix = isM ? COV_O_C + pi : COV_REC - 1;   // (the last double of a record is 0)
    const bool vec = isM || isMu || isDu;               // the state "rows" are the means
    const int sX = vec ? LQC_M : LQC_X + pj * 6, sC = vec ? LQC_MU : LQC_C + pj * 6;
    const int sCT = vec ? LQC_M : LQC_CT + pj * 6, sE = vec ? LQC_MU : LQC_E + pj * 6;
    const int dC1 = isP ? LQC_Y1 + L : (isM ? LQC_ST + LQC_M + pi : (isDu ? LQC_O + kr : (isKH ? LQC_KH + (L - 50) : LQC_DUMP)));
    const int dC2 = isP ? LQC_Y2 + L : LQC_DUMP;
    const int dC3 = isP ? LQC_Y3 + L : (isMu ? LQC_ST + LQC_MUM + pi : LQC_DUMP);   // (+ LQC_ST: the other parity)
    // round D: rows of Y (or of K H), the right rows F_b (or K_s), A_j, A_b
    const int sD1 = isQ ? LQC_KH + qr * 6 : LQC_Y1 + pa * 6, sD2 = LQC_Y2 + pa * 6, sD3 = LQC_Y2 + pi * 6, sD4 = LQC_Y3 + pa * 6;
    const int oF2 = isQ ? COV_O_K + qs * 6 : pb * 6, oA2 = pj * 6, oA3 = pb * 6;
    const int dD1 = isP ? LQC_ST + LQC_X + L : (isQ ? LQC_O + 2 + (L - 36) : LQC_DUMP);
    const int dD2 = isP ? LQC_ST + LQC_CM + L : LQC_DUMP, dD3 = isP ? LQC_ST + LQC_EM + L : LQC_DUMP;
    const real w = (isP && pi == pj) ? (real)W.w[pi] : R(0.0);
    // the record's entries this lane stores: L and, on lanes 0-31, 64 + L
    auto entry = [](int e) {
        if (e < 6) return LQC_M + e;
        if (e < 12) return LQC_MU + (e - 6);
        if (e < 54) {
            int q = e < 33 ? e - 12 : e - 33, i = 0;
            while (q >= 6 - i) { q -= 6 - i; i++; }
            return (e < 33 ? LQC_X : LQC_E) + i * 6 + i + q;
        }
        if (e < 90) return LQC_C + (e - 54);
        if (e < 95) return LQC_O + (e - 90);
        return LQC_ZERO;
    };
    const int src0 = entry(L), src1 = entry(L < 32 ? 64 + L : 95);
    const bool in1 = L >= 26 && L < 31;   // entries 90-94: the input moments

    real pfF[COV_PF], pfA[COV_PF], pfL[LQC_LPF];
    int dstA[COV_PF];   // where this lane's doubles of a block of k_cov_stage<false>'s records go in shA
#pragma unroll
    for (int i = 0; i < COV_PF; i++) {
        const int e = i * TILE + L, smp = e / COV_REC, r = e % COV_REC;
        dstA[i] = r < 36 ? smp * LQC_AREC + r : (r == COV_O_FLAG ? smp * LQC_AREC + LQC_A_FLAG : COV_BLK * LQC_AREC);
    }
    bool bad = false;
    auto fetch = [&](int b) {
        cov_fetch(rcF, nrec, b, L, pfF);
        cov_fetch(rcA, nrec, b, L, pfA);
#pragma unroll
        for (int i = 0; i < LQC_LPF; i++) {
            const size_t e = (size_t)b * COV_BLK * LQC_LREC + i * TILE + L;
            pfL[i] = rcL[e < nl ? e : nl - 1];
            bad = bad || !__builtin_isfinite(pfL[i]);
        }
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int i = 0; i < LQC_LPF; i++) shL[b & 1][i * TILE + L] = pfL[i];
#pragma unroll
        for (int i = 0; i < COV_PF; i++) shA[b & 1][dstA[i]] = pfA[i];
        cov_stash(shF[b & 1], L, pfF);   // (its barrier orders all three)
    };
    // record t_out (everything under the parity of t_out) goes out
    auto emit = [&](int t_out, bool inputs) {
        const real* st = &ws[(t_out & 1) * LQC_ST];
        real* __restrict__ out = pred + ((size_t)opt * T + t_out) * LQC_NREC;
        out[L] = st[src0];
        if (L < 32) out[64 + L] = (in1 && !inputs) ? R(0.0) : st[src1];
    };
    // J row `r` from the same row of L
    auto jrow = [](const real l[6], int r, real j[6]) {
#pragma unroll
        for (int k = 0; k < 6; k++) j[k] = (k == r ? R(1.0) : R(0.0)) - l[k];
    };
    // The measurement update of sample t: rounds A and B; the record of sample t - 1 leaves in between.
    auto measure = [&](int t, const real* __restrict__ rl) {
        real* st = &ws[(t & 1) * LQC_ST];
        real li[6], lj[6], la[6], lb[6], ji[6], jj[6], jb[6], lv[6], x1[6], x2[6], g[6];
        row6(rl + pi * 6, li);          // the stream: nothing here waits for the previous stage
        row6(rl + pj * 6, lj);
        row6(rl + pa * 6, la);
        row6(rl + pb * 6, lb);
        jrow(li, pi, ji);
        jrow(lj, pj, jj);
        jrow(lb, pb, jb);
#pragma unroll
        for (int k = 0; k < 6; k++) lv[k] = la[k] * (real)V.w[k];
        const real lvl = dot6(lv, lb, R(0.0));
        __syncthreads();                // the prior state of sample t and everything of sample t - 1 are in LDS
        row6(st + sA1, x1);
        row6(st + sA2, x2);
        if (t > 0) emit(t - 1, true);
        const real ga = dot6(ji, x1, R(0.0)), cn = dot6(x2, jj, R(0.0));
        st[dA1] = ga;
        st[dA2] = cn;
        st[dA3] = cn;
        __syncthreads();
        row6(st + sB, g);
        st[dB] = dot6(g, jb, lvl);
    };

    // ---- sample 0 ----
    {
        real s0 = R(0.0), m0 = R(0.0), e0 = R(0.0);
        if (isP && Sigma0) s0 = Sigma0[(size_t)opt * 21 + sidx(pa, pb)];
        if (isM && mean0) m0 = mean0[(size_t)opt * 6 + pi];
        if (isM && ehat0) e0 = ehat0[(size_t)opt * 6 + pi];
        if (isP) { ws[LQC_X + L] = s0; ws[LQC_CM + L] = s0; ws[LQC_EM + L] = s0; }
        if (isM) { ws[LQC_M + pi] = m0; ws[LQC_MUM + pi] = m0 - e0; }
        if (L < 2) { ws[LQC_ZERO + L] = R(0.0); ws[LQC_ST + LQC_ZERO + L] = R(0.0); }   // entry 95: +0.0 for good
    }
    int flags = 0;
    fetch(0);
    stash(0);
    for (int b = 0, t0 = 0; t0 < T - 1; b++, t0 += COV_BLK) {
      fetch(b + 1);   // in flight during the COV_BLK stages below
      const int n = T - 1 - t0 < COV_BLK ? T - 1 - t0 : COV_BLK;
      for (int i = 0; i < n; i++) {
        const int t = t0 + i;
        const real* __restrict__ rf = &shF[b & 1][i * COV_REC];
        const real* __restrict__ ra = &shA[b & 1][i * LQC_AREC];
        const real* st = &ws[(t & 1) * LQC_ST];
        // a destination d >= LQC_ST lies under the other parity: the state of sample t + 1
        auto dst = [&](int d) -> real& { return ws[d >= LQC_ST ? ((t + 1) & 1) * LQC_ST + (d - LQC_ST) : (t & 1) * LQC_ST + d]; };
        real f1[6], a1[6], n1[6], f2[6], a2[6], a3[6], n2[6];
        row6(rf + oF1, f1);             // the stream
        row6(ra + oA1, a1);
        row6(rf + oF2, f2);
        row6(ra + oA2, a2);
        row6(ra + oA3, a3);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            n1[k] = useK ? f1[k] : f1[k] - a1[k];
            n2[k] = f2[k] - a3[k];
        }
        const real cadd = rf[cix];
        flags |= (int)rf[COV_O_FLAG] | (int)ra[LQC_A_FLAG];
        measure(t, &shL[b & 1][i * LQC_LREC]);
        __syncthreads();                // the posterior state of sample t is in LDS
        // ---- round C ----
        real x[6], c[6], ct[6], e[6];
        row6(st + sX, x);
        row6(st + sC, c);
        row6(st + sCT, ct);
        row6(st + sE, e);
        const real y1 = dot6(f1, x, R(0.0)) - dot6(n1, c, R(0.0));
        const real y2 = dot6(f1, ct, R(0.0)) - dot6(n1, e, R(0.0));
        const real y3 = dot6(a1, e, R(0.0));
        // (the destinations of the other parity hold the record of sample t - 1, which left in round A)
        dst(dC1) = isKH ? y1 - y2 : y1 + cadd;
        dst(dC2) = y2;
        dst(dC3) = y3;
        __syncthreads();
        // ---- round D ----
        real r1[6], r2[6], r3[6], r4[6];
        row6(st + sD1, r1);
        row6(st + sD2, r2);
        row6(st + sD3, r3);
        row6(st + sD4, r4);
        const real p1 = dot6(r1, f2, R(0.0)), p2 = dot6(r2, n2, R(0.0));
        dst(dD1) = isQ ? p1 : (p1 - p2) + w;
        dst(dD2) = dot6(r3, a2, w);
        dst(dD3) = dot6(r4, a3, w);
      }
      stash(b + 1);
    }
    {
        const int bl = (T - 1) / COV_BLK, il = (T - 1) % COV_BLK;
        flags |= (int)shF[bl & 1][il * COV_REC + COV_O_FLAG] | (int)shA[bl & 1][il * LQC_AREC + LQC_A_FLAG];
        measure(T - 1, &shL[bl & 1][il * LQC_LREC]);   // (and the record of sample T - 2 leaves)
    }
    __syncthreads();
    emit(T - 1, false);
    if (__any(bad)) flags |= AOC_ST_NAN;
    if (L == 0 && status && flags) status[opt] |= flags;
}

#ifndef AOC_KERNELS_ONLY
// aoc_track_covariance_lqg_scratch_bytes: the records of both k_cov_stage instances, 2 x [n_opt][T][COV_REC]; 0 for a
// geometry the call refuses anyway
static size_t track_covariance_lqg_scratch_bytes(int32_t n_opt, int32_t T) { return 2 * track_covariance_scratch_bytes(n_opt, T); }

// Body of aoc_track_covariance_lqg.  A template only so that the kernels it names are instantiated where it is called — from
// the fp64 entry point — and not once more in the float32 namespace.
template <typename = void>
static int api_track_covariance_lqg(const aoc_problem* p, int32_t n_opt, const real* nominal, const real* filter,
                                    const real* mean0, const real* ehat0, const real* Sigma0, const aoc_mpc_noise* noise,
                                    const double* rho, real* pred, int32_t* status, void* scratch, size_t scratch_bytes) {
    const char* fn = "aoc_track_covariance_lqg";
    if (!p) return einval("%s: aoc_problem is NULL", fn);
    if (!nominal) return einval("%s: nominal is NULL", fn);
    if (!filter) return einval("%s: filter is NULL", fn);
    if (!pred) return einval("%s: pred is NULL", fn);
    if (n_opt < 1) return einval("%s: n_opt = %d (need n_opt >= 1)", fn, n_opt);
    if (p->T < 3) return einval("%s: T = %d (need T >= 3)", fn, p->T);
    CovW W, V;
    for (int c = 0; c < 6; c++) {
        const double r = rho ? rho[c] : 0.0, s = noise ? noise->sigma[c] : 0.0;
        if (!(r >= 0.0) || !__builtin_isfinite(r)) return einval("%s: rho[%d] = %g (need a finite rho >= 0)", fn, c, r);
        if (!(s >= 0.0) || !__builtin_isfinite(s)) return einval("%s: sigma[%d] = %g (need a finite sigma >= 0)", fn, c, s);
        V.w[c] = r * r;
        W.w[c] = s * s;
    }
    const size_t need = track_covariance_lqg_scratch_bytes(n_opt, p->T);
    if (!scratch) return einval("%s: scratch is NULL (need %zu bytes, aoc_track_covariance_lqg_scratch_bytes)", fn, need);
    if ((uintptr_t)scratch % 16) return einval("%s: scratch must be 16-byte aligned", fn);
    if (scratch_bytes < need)
        return einval("%s: scratch_bytes = %zu, need %zu (aoc_track_covariance_lqg_scratch_bytes)", fn, scratch_bytes, need);
    KConst k = make_const(p->model, nullptr, nullptr, nullptr, n_opt, p->T);
    hipStream_t st = (hipStream_t)p->stream;
    const size_t total = (size_t)n_opt * p->T;
    real* recF = (real*)scratch;
    real* recA = recF + total * COV_REC;
    const dim3 grid((unsigned)((total + COV_THREADS - 1) / COV_THREADS));
    hipLaunchKernelGGL(k_cov_stage<true>, grid, dim3(COV_THREADS), 0, st, k, n_opt, nominal, recF);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(k_cov_stage<false>, grid, dim3(COV_THREADS), 0, st, k, n_opt, nominal, recA);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(k_lqgcov_chain<>, dim3(n_opt), dim3(TILE), 0, st, p->T, (const real*)recF, (const real*)recA, filter,
                       mean0, ehat0, Sigma0, W, V, pred, status);
    return check_launch(fn);
}
#endif  // AOC_KERNELS_ONLY
