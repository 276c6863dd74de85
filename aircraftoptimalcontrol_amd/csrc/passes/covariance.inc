// passes/covariance.inc — linear covariance prediction for a closed-loop tracking ensemble (aoc_track_covariance).
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// What linear theory predicts for the loop of ensemble.inc about one optimum: with A_t, B_t the Jacobians of the plant step
// at (x_opt_t, u_opt_t), F_t = A_t + B_t K_t and c_t = step(x_opt_t, u_opt_t) - x_opt_{t+1},
//     m_{t+1} = F_t m_t + c_t,      P_{t+1} = F_t P_t F_t^T + W,      W = diag(sigma^2),
// from m_0 = mean0, P_0 = Sigma0, and per sample the moments of the input deviation K_t m_t, K_t P_t K_t^T.  The record
// of one (optimum, sample), COV_NREC = AOC_COV_NREC = 32 doubles: m[6], the upper triangle of P row by row [21] (the order
// of the envelope's entries 23-43), K m [2], K P K^T (00, 01, 11) [3]; sample T-1 has no input: +0.0 there.
//
// Two kernels, split by what depends on the previous stage:
//   k_cov_stage   one lane per (optimum, sample): sin/cos, linearise, step_state, F_t and c_t — everything a stage needs
//                 that does NOT depend on P or m — into scratch, COV_REC doubles per sample:
//                     F row-major [36], c [6], K row 0 [6], K row 1 [6], status bits of this sample (as a double), 0.
//                 T lanes per optimum: wide for any n_opt.
//   k_cov_chain   one wavefront per optimum, serial in t, the LANES own the entries: lane 6i+j the entry (i,j) of P,
//                 lane 36+i the entry i of m, and the input moments ride along on lanes 42-58.  A stage is two rounds of
//                 6-term products, y = (left row) . (state column), then z = (y row) . (right row):
//                     lane         round 1: y =                     round 2: z =                       keeps
//                     6i+j         F_i. P_.j    = (F P)_ij          (F P)_a. F_b. + W_ab, a<=b         P'_ij = z
//                     36+i         F_i. m + c_i = m'_i              -                                  m'_i = y
//                     42+r         K_r. m       = (K m)_r           -                                  record 27+r = y
//                     44+6r+j      K_r. P_.j    = (K P)_rj          -                                  -
//                     56+q         -                                (K P)_r. K_s.,  (r,s) = q-th of 00, 01, 11   record 29+q = z
//                 The lanes (i,j) and (j,i) evaluate the SAME expression of round 2 (a = min, b = max), so P stays
//                 symmetric bit for bit and no asymmetry can build up; round 1 reads column j of P as row j.
//                 Operands of other lanes travel through LDS: state and y are written, then read back as three
//                 ds_read_b128 per round.  (Cross-lane moves instead — twelve ds_bpermute_b32 per round, no write on the
//                 chain — were measured and are slower: 0.245 against 0.222 ms for one optimum and T = 800, 0.549 against
//                 0.424 ms for 1024 optima; EXPERIMENTS.md.)  The records of k_cov_stage are a pure stream, fetched a
//                 block of COV_BLK samples ahead into an LDS double buffer like the nominal of k_track_ensemble.  The
//                 record of a sample leaves as one coalesced 256-byte store of lanes 0-31, gathered from LDS one stage
//                 later, off the chain.
// Every sum starts from +0.0 and is a chain of fused multiply-adds, so with P_0 = 0 and W = 0 every covariance entry is
// exactly +0.0 wherever F is finite.  No atomics; an optimum's bits depend on nothing but its own inputs.
// Only the fp64 build launches these kernels: the templates are never instantiated in the float namespace.
// ---------------------------------------------------------------------------------------------
constexpr int COV_NREC = 32;    // AOC_COV_NREC
constexpr int COV_REC = 56;     // doubles per sample in scratch
constexpr int COV_BLK = 16;     // samples per cooperative load
constexpr int COV_PF = COV_BLK * COV_REC / TILE;   // doubles per lane and block
constexpr int COV_O_C = 36, COV_O_K = 42, COV_O_FLAG = 54;   // offsets of c, K and the status bits in a scratch record
constexpr int COV_THREADS = 64;
static_assert(COV_PF * TILE == COV_BLK * COV_REC, "a block of records is a whole number of doubles per lane");
static_assert(COV_REC % 2 == 0 && COV_O_K % 2 == 0, "rows of F and K start on 16 bytes");

struct CovW { double w[6]; };   // sigma^2

// BK = false (filter.inc): the record holds A_t instead of F_t — a filter knows its input — and the gains, which it does not
// read, do not count as entries of the optimum's record.
// BENT = true (the limited LQG loop of lqg.inc, which never reads the record's copy of K): the two entries of B_t that depend
// on the optimum, b20 and b50, lie where row 0 of that copy starts (COV_O_K, COV_O_K + 1); everything else is what it was.
template <bool BK = true, bool BENT = false>
__global__ __launch_bounds__(COV_THREADS) void k_cov_stage(KConst k, int n_opt, const real* __restrict__ nominal,
                                                           real* __restrict__ rec) {
    const int T = k.T;
    const size_t idx = (size_t)blockIdx.x * COV_THREADS + threadIdx.x;
    if (idx >= (size_t)n_opt * T) return;
    const int t = (int)(idx % T);
    const real* __restrict__ nm = nominal + idx * ENS_REC;
    real v[ENS_REC], xnext[6], xp[6];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < ENS_REC; j++) {
        v[j] = nm[j];
        if (BK || j < 8) fin = fin && __builtin_isfinite(v[j]);
    }
#pragma unroll
    for (int c = 0; c < 6; c++) xnext[c] = t < T - 1 ? nm[ENS_REC + c] : v[c];
    int flags = fin ? 0 : AOC_ST_NAN;
    if (t < T - 1 && !(v[2] > R(0.0))) flags |= AOC_ST_VNONPOS;
    const real u0 = v[6], u1 = v[7];
    const SC s = trig(v[3], v[5]);
    step_state(k, v, u0, u1, s, xp);   // the plant's own arithmetic, float32 rounding included
    const Lin l = linearise(k, v, u0, s);
    real F[36];
#pragma unroll
    for (int e = 0; e < 36; e++) F[e] = R(0.0);
    F[0] = R(1.0); F[7] = R(1.0); F[21] = R(1.0); F[28] = R(1.0); F[3 * 6 + 4] = k.dt;
    F[0 * 6 + 2] = l.a02; F[0 * 6 + 5] = l.a05; F[1 * 6 + 2] = l.a12; F[1 * 6 + 5] = l.a15;
    F[2 * 6 + 2] = l.a22; F[2 * 6 + 3] = l.a23; F[2 * 6 + 5] = l.a25;
    F[5 * 6 + 2] = l.a52; F[5 * 6 + 3] = l.a53; F[5 * 6 + 5] = l.a55;
    if constexpr (BK) {
#pragma unroll
        for (int j = 0; j < 6; j++) {   // F = A + B K: B has the entries (2,0), (5,0) and (4,1)
            F[2 * 6 + j] = fma_r(l.b20, v[8 + j], F[2 * 6 + j]);
            F[5 * 6 + j] = fma_r(l.b50, v[8 + j], F[5 * 6 + j]);
            F[4 * 6 + j] = fma_r(k.b41, v[14 + j], F[4 * 6 + j]);
        }
    }
    real2v* __restrict__ out = (real2v*)(rec + idx * COV_REC);
#pragma unroll
    for (int e = 0; e < 18; e++) out[e] = real2v{F[2 * e], F[2 * e + 1]};
#pragma unroll
    for (int e = 0; e < 3; e++) out[COV_O_C / 2 + e] = real2v{xp[2 * e] - xnext[2 * e], xp[2 * e + 1] - xnext[2 * e + 1]};
#pragma unroll
    for (int e = 0; e < 6; e++) out[COV_O_K / 2 + e] = (BENT && e == 0) ? real2v{l.b20, l.b50} : real2v{v[8 + 2 * e], v[9 + 2 * e]};
    out[COV_O_FLAG / 2] = real2v{(real)flags, R(0.0)};
}

// What the chain kernels (k_cov_chain here, k_filter_chain of filter.inc) share.  The stream of k_cov_stage's records: block b
// = the records of the samples b*COV_BLK .., COV_PF doubles per lane, clamped onto the optimum's last double; fetched into
// registers a block ahead, then stashed into one half of an LDS double buffer.
__device__ __forceinline__ void cov_fetch(const real* __restrict__ rc, size_t nrec, int b, int L, real pf[COV_PF]) {
#pragma unroll
    for (int i = 0; i < COV_PF; i++) {
        const size_t e = (size_t)b * COV_BLK * COV_REC + i * TILE + L;
        pf[i] = rc[e < nrec ? e : nrec - 1];
    }
}
__device__ __forceinline__ void cov_stash(real* __restrict__ half, int L, const real pf[COV_PF]) {
#pragma unroll
    for (int i = 0; i < COV_PF; i++) half[i * TILE + L] = pf[i];
    __syncthreads();   // one wavefront: orders the LDS writes before the reads
}
// a 6-term product from +0.0, two chains of three fused multiply-adds, plus `add`
__device__ __forceinline__ real dot6(const real a[6], const real b[6], real add) {
    const real s0 = fma_r(a[2], b[2], fma_r(a[1], b[1], fma_r(a[0], b[0], R(0.0))));
    const real s1 = fma_r(a[5], b[5], fma_r(a[4], b[4], fma_r(a[3], b[3], R(0.0))));
    return (s0 + s1) + add;
}
// six consecutive values, 16-byte aligned: three ds_read_b128
__device__ __forceinline__ void row6(const real* __restrict__ p, real out[6]) {
    const real2v* __restrict__ q = (const real2v*)p;
#pragma unroll
    for (int e = 0; e < 3; e++) { const real2v v2 = q[e]; out[2 * e] = v2.x; out[2 * e + 1] = v2.y; }
}

// LDS of k_cov_chain beside the stream's double buffer: st[2][48] the state (P full [36], m [6]) of even / odd samples,
// o[8] the input moments of the sample last finished, y[64] the results of round 1 (lane L at y[L]), one slot to spare for
// the lanes that own nothing.
constexpr int COV_ST = 48, COV_O = 2 * COV_ST, COV_Y = COV_O + 8, COV_DUMP = COV_Y + TILE, COV_LDS = COV_DUMP + 2;

template <typename = void>
__global__ __launch_bounds__(TILE) void k_cov_chain(int T, const real* __restrict__ rec, const real* __restrict__ mean0,
                                                    const real* __restrict__ Sigma0, CovW W, real* __restrict__ pred,
                                                    int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real sh[2][COV_BLK * COV_REC];
    __shared__ __attribute__((aligned(16))) real ws[COV_LDS];
    const int opt = blockIdx.x, L = threadIdx.x;
    const real* __restrict__ rc = rec + (size_t)opt * T * COV_REC;   // wave-uniform
    const size_t nrec = (size_t)T * COV_REC;
    // ---- what this lane computes (fixed for the whole kernel) ----
    const bool isP = L < 36, isM = L >= 36 && L < 42, isKm = L >= 42 && L < 44, isKP = L >= 44 && L < 56,
               isQ = L >= 56 && L < 59;
    const int pi = isP ? L / 6 : 0, pj = isP ? L % 6 : 0, pa = pi < pj ? pi : pj, pb = pi < pj ? pj : pi;
    const int kr = isKm ? L - 42 : (isKP ? (L - 44) / 6 : 0), kj = isKP ? (L - 44) % 6 : 0;
    const int qr = L == 58 ? 1 : 0, qs = L == 56 ? 0 : 1;
    // round 1: left row in the record, column of the state (P row j, or m)
    const int l1 = isP ? pi * 6 : (isM ? (L - 36) * 6 : COV_O_K + kr * 6);
    const int r1 = isP ? pj * 6 : (isKP ? kj * 6 : 36);
    const int cix = isM ? COV_O_C + (L - 36) : COV_REC - 1;   // (the last double of a record is 0)
    // round 2: row of y, right row in the record
    const int l2 = isP ? pa * 6 : (isQ ? 44 + qr * 6 : 0);
    const int r2 = isP ? pb * 6 : COV_O_K + qs * 6;
    const real w = (isP && pi == pj) ? (real)W.w[pi] : R(0.0);
    // where the result goes: the state of the next sample, the input moments, or nowhere
    const int dst_o = isKm ? COV_O + (L - 42) : (isQ ? COV_O + 2 + (L - 56) : COV_DUMP);
    // the record's entry this lane stores (lanes 0-31): m, the upper triangle of P, the input moments
    int src = COV_DUMP;
    bool src_state = false;
    if (L < 6) { src = 36 + L; src_state = true; }
    else if (L < 27) {
        int e = L - 6, i = 0;
        while (e >= 6 - i) { e -= 6 - i; i++; }
        src = i * 6 + i + e;
        src_state = true;
    } else if (L < 32) src = COV_O + (L - 27);

    real pf[COV_PF];
    auto fetch = [&](int b) { cov_fetch(rc, nrec, b, L, pf); };
    auto stash = [&](int b) { cov_stash(sh[b & 1], L, pf); };
    // record t - 1 (state of parity (t - 1) & 1, the input moments as they lie) goes out
    auto emit = [&](int t_out, bool inputs) {
        if (L < COV_NREC) {
            real v = ws[src + (src_state ? (t_out & 1) * COV_ST : 0)];
            if (!inputs && L >= 27) v = R(0.0);
            pred[((size_t)opt * T + t_out) * COV_NREC + L] = v;
        }
    };

    // ---- sample 0 ----
    real val = R(0.0);   // this lane's entry of the state at sample 0
    if (isP && Sigma0) val = Sigma0[(size_t)opt * 21 + sidx(pa, pb)];
    if (isM && mean0) val = mean0[(size_t)opt * 6 + (L - 36)];
    if (L < 42) ws[L] = val;
    int flags = 0;
    fetch(0);
    stash(0);
    for (int b = 0, t0 = 0; t0 < T - 1; b++, t0 += COV_BLK) {
      fetch(b + 1);   // in flight during the COV_BLK stages below
      const int n = T - 1 - t0 < COV_BLK ? T - 1 - t0 : COV_BLK;
      for (int i = 0; i < n; i++) {
        const int t = t0 + i;
        const real* __restrict__ rn = &sh[b & 1][i * COV_REC];
        real a1[6], b2[6], x1[6], x2[6];
        row6(rn + l1, a1);            // the stream: nothing here waits for the previous stage
        row6(rn + r2, b2);
        const real cadd = rn[cix];
        flags |= (int)rn[COV_O_FLAG];
        __syncthreads();              // the state of sample t and the moments of t - 1 are in LDS
        row6(&ws[(t & 1) * COV_ST + r1], x1);
        if (t > 0) emit(t - 1, true);
        const real y = dot6(a1, x1, cadd);
        ws[COV_Y + L] = y;
        __syncthreads();              // (and record t - 1 is read before its slots are written again below)
        row6(&ws[COV_Y + l2], x2);
        const real z = dot6(x2, b2, w);
        ws[L < 42 ? ((t + 1) & 1) * COV_ST + L : dst_o] = (isP || isQ) ? z : y;
      }
      stash(b + 1);
    }
    __syncthreads();
    emit(T - 2, true);
    emit(T - 1, false);
    flags |= (int)sh[((T - 1) / COV_BLK) & 1][((T - 1) % COV_BLK) * COV_REC + COV_O_FLAG];
    if (L == 0 && status && flags) status[opt] |= flags;
}

#ifndef AOC_KERNELS_ONLY
// aoc_track_covariance_scratch_bytes: rec[n_opt][T][COV_REC]; 0 for a geometry the call refuses anyway
static size_t track_covariance_scratch_bytes(int32_t n_opt, int32_t T) {
    if (n_opt < 1 || T < 3) return 0;
    return (size_t)n_opt * (size_t)T * COV_REC * sizeof(double);
}

// Body of aoc_track_covariance.  A template only so that the kernels it names are instantiated where it is called — from
// the fp64 entry point — and not once more in the float32 namespace.
template <typename = void>
static int api_track_covariance(const aoc_problem* p, int32_t n_opt, const real* nominal, const real* mean0,
                                const real* Sigma0, const aoc_mpc_noise* noise, real* pred, int32_t* status, void* scratch,
                                size_t scratch_bytes) {
    const char* fn = "aoc_track_covariance";
    if (!p) return einval("%s: aoc_problem is NULL", fn);
    if (!nominal) return einval("%s: nominal is NULL", fn);
    if (!pred) return einval("%s: pred is NULL", fn);
    if (n_opt < 1) return einval("%s: n_opt = %d (need n_opt >= 1)", fn, n_opt);
    if (p->T < 3) return einval("%s: T = %d (need T >= 3)", fn, p->T);
    const size_t need = track_covariance_scratch_bytes(n_opt, p->T);
    if (!scratch) return einval("%s: scratch is NULL (need %zu bytes, aoc_track_covariance_scratch_bytes)", fn, need);
    if ((uintptr_t)scratch % 16) return einval("%s: scratch must be 16-byte aligned", fn);
    if (scratch_bytes < need)
        return einval("%s: scratch_bytes = %zu, need %zu (aoc_track_covariance_scratch_bytes)", fn, scratch_bytes, need);
    KConst k = make_const(p->model, nullptr, nullptr, nullptr, n_opt, p->T);
    CovW W;
    for (int c = 0; c < 6; c++) W.w[c] = noise ? noise->sigma[c] * noise->sigma[c] : 0.0;
    hipStream_t st = (hipStream_t)p->stream;
    const size_t total = (size_t)n_opt * p->T;
    hipLaunchKernelGGL(k_cov_stage<>, dim3((unsigned)((total + COV_THREADS - 1) / COV_THREADS)), dim3(COV_THREADS), 0, st, k,
                       n_opt, nominal, (real*)scratch);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(k_cov_chain<>, dim3(n_opt), dim3(TILE), 0, st, p->T, (const real*)scratch, mean0, Sigma0, W, pred,
                       status);
    return check_launch(fn);
}
#endif  // AOC_KERNELS_ONLY
