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

// ---- per-stage envelope over the members (aoc_track_ensemble_envelope) ----------------------------------------------
// Record of one (optimum, sample): n, min / max of dx[6] and du[2], sum dx[6], sum dx_i dx_j (i <= j), AOC_ENV_NREC = 44
// doubles (include/aoc.h).  The ENV instances of k_track_ensemble stage ENV_S samples at a time in LDS, ENV_ROWS rows
// of one value per member each,
//     0-5 dx[c]   6-7 du[r]   8 one = 1.0   9 pen = 0.0      for a member that counts,
//     0-5 0.0     6-7 0.0     8 one = 0.0   9 pen = +inf     for one that does not (selected, never multiplied: its NaN
//                                                            stays in its lane),
// and then turn the work round: lane L reduces ITEM L over the 64 members.  With v = (dx0..dx5, one) every sum of the
// record is a sum of v_i v_j over the members — n = one.one, sum dx_i = dx_i.one, the moments dx_i.dx_j — 28 pairs per
// sample, dealt as 14 tasks (a; b, c) = the pairs (a,b) and (a,c) that share row a: three LDS reads and two fused
// multiply-adds per member, in member order 0..63 (the order is fixed, so are the bits; one.one and dx.one are exact).
// ENV_S samples x 14 tasks occupy 56 lanes.  min / max: lane L = (sample L/16, quantity (L/2)%8, half L%2 of the members)
// folds min(v + pen) and max(v - pen), the halves meet through one shuffle.  The item lanes read two members at a time
// (ds_read_b128: 256 B per LDS cycle; the ds_read2_b64 the compiler makes of 8-byte reads runs at half that), so rows are
// 16-byte aligned, ENV_LD = 66 doubles apart: lanes on different rows and one column meet on a bank only where their
// rows are 16 apart.  Each tile's records go to `part[tile][t][44]`; k_envelope_fold folds the tiles of an optimum in tile order.
constexpr int ENV_NREC = 44;    // AOC_ENV_NREC
constexpr int ENV_S = 4;        // samples staged per reduction
constexpr int ENV_ROWS = 10;
constexpr int ENV_LD = TILE + 2;
constexpr int ENV_NTASK = 14;
static_assert(ENV_S * ENV_NTASK <= TILE && ENV_S * 16 == TILE, "one reduction occupies one wavefront");
static_assert(ENS_BLK % ENV_S == 0, "a block of stage records is a whole number of envelope blocks");

// index in the record of the sum over the members of v_i v_j, v = (dx0..dx5, one)
__host__ __device__ constexpr int env_rec(int i, int j) {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return hi == 6 ? (lo == 6 ? 0 : 17 + lo) : 23 + lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
}
// task k = (a, b, c), four bits each: the 28 pairs of the upper triangle of v v^T, two per task, sharing row a
__host__ __device__ constexpr unsigned env_task(int k) {
    constexpr unsigned t[ENV_NTASK] = {0x001, 0x023, 0x045, 0x112, 0x134, 0x156, 0x223, 0x245, 0x334, 0x356, 0x445, 0x556,
                                       0x602, 0x646};
    return t[k];
}
constexpr bool env_tasks_cover() {
    bool seen[ENV_NREC] = {};
    int n = 0;
    for (int k = 0; k < ENV_NTASK; k++) {
        const int a = env_task(k) >> 8, b = (env_task(k) >> 4) & 15, c = env_task(k) & 15;
        for (int r : {env_rec(a, b), env_rec(a, c)}) {
            if (r < 0 || r >= ENV_NREC || seen[r]) return false;
            seen[r] = true;
            n++;
        }
    }
    return n == 28 && seen[0] && !seen[1] && !seen[16] && seen[17] && seen[43];
}
static_assert(env_tasks_cover(), "the 14 tasks are the 28 sums of the record, each once");

// ---- per-sample histogram over the members (aoc_track_ensemble_histogram) ---------------------------------------------
// hist[opt][t][c][k], c = dx[0..5], du[0..1], k = bin of s = (v - lo) * inv_w under bins[opt][t][c] = (lo, inv_w)
// (include/aoc.h).  The 16 doubles of a stage's bins travel like the nominal's record: HIST_PF coalesced doubles per lane
// a block ahead into LDS, read back as eight ds_read_b128 at one address for all lanes (block b = the records
// b*ENS_BLK .. of the SAME stages: bins are used where the stage starts, not a stage ahead).  A tile has 64 members, so a
// count of a tile fits a byte: the HIST instances keep, per sample slot and channel, 64 byte counters as 16 dwords in LDS,
// and a lane that counts adds 1 << 8 (k % 4) to dword k / 4 with one returnless ds_add_u32 — no carry can cross a byte
// (at most 64 adds of 1 each).  The counters ARE the tile's partial part[tile][t][c][64 bytes]: every HIST_S samples the
// wavefront copies them out as they lie, 16 bytes per lane and instruction (ds_read_b128 / global store / ds_write_b128 of
// zeros, all conflict-free and coalesced), and k_histogram_fold adds the tiles of an optimum into int32.
constexpr int HIST_NCH = 8;     // AOC_HIST_NCH
constexpr int HIST_NBIN = 64;   // AOC_HIST_NBIN
constexpr int HIST_REC = 2 * HIST_NCH;              // doubles per stage of `bins`
constexpr int HIST_PF = ENS_BLK * HIST_REC / TILE;  // doubles per lane and block
constexpr int HIST_S = 8;                           // samples between two drains
constexpr int HIST_DW = HIST_NCH * HIST_NBIN / 4;   // dwords of byte counters per sample (and tile)
constexpr int HIST_DRAIN = HIST_S * HIST_DW / 4 / TILE;   // 16-byte pieces per lane and drain
static_assert(HIST_PF * TILE == ENS_BLK * HIST_REC, "a block of bins is a whole number of doubles per lane");
static_assert(HIST_DRAIN * TILE * 4 == HIST_S * HIST_DW, "a drain is a whole number of 16-byte pieces per lane");
static_assert(TILE <= 255, "a tile's count fits a byte");

// ---- noisy measurements and a Kalman estimate in the loop (aoc_track_ensemble_lqg) ------------------------------------------
// The EST instances of k_track_ensemble feed back an estimate instead of the true deviation.  With dx_t = x_t - x_opt_t, the
// measurement y_t = dx_t + v_t and e^-_0 = ehat0 of the optimum, sample t = 0 .. T-1 does
//     e^+_t = e^-_t + L_t (y_t - e^-_t),      u_t = u_opt_t + K_t e^+_t,      e^-_{t+1} = F_t e^+_t + c_t      (t <= T-2),
// F_t = A_t + B_t K_t and c_t the records of k_cov_stage (covariance.inc; launched into the call's scratch by lqg.inc), L_t
// the caller's filter gains: all three depend on the optimum only, so they reach the lanes through LDS like the nominal —
// EST_FC_PF + EST_L_PF coalesced doubles per lane and block of ENS_BLK stages (block b = the records of the SAME stages
// b*ENS_BLK ..), read back with every lane at one address.  The whole record of k_cov_stage is staged as it lies (a
// contiguous stream; its copy of K and its status word are not read).  Unlike the nominal this block is NOT prefetched
// through registers and NOT double-buffered: 23 doubles per lane held over a block of stages are 46 VGPRs on top of instances
// that already fill the register file (the first form spilled to private scratch), and a stage takes 1500-5000 cycles
// against one exposed load (an L2 hit: every tile of the optimum reads the same records) per sixteen stages.  So the block is loaded and written between two blocks of
// stages: 16 x (56 + 36) doubles = 11.5 KB beside the nominal's 5 KB.
// The estimate is six registers per lane.  L (y - e^-) and F e^+ are chains of fused multiply-adds from +0.0 in index order,
// added to e^- resp. c once: with L = 0 and c = 0 the estimate stays exactly +0.0.  v_t[c] = rho[c] z from the generator of
// the disturbance with the counter's fourth word 1 (mpc_noise_draw), drawn only where rho draws, else +0.0.
// est_stats[tile][EST_NSTAT][64]: 0-5 max_t |e_t[c]| of e_t = dx_t - e^+_t (a NaN sticks), 6-11 sum_t e_t[c]^2 in sample order.
constexpr int EST_FC = 56;      // doubles per sample of the F / c records (COV_REC, asserted in lqg.inc) ...
constexpr int EST_O_C = 36;     // ... and where c starts in one (COV_O_C)
constexpr int EST_L = 36;       // doubles per sample of `filter`
constexpr int EST_NSTAT = 12;   // AOC_LQG_NSTAT
constexpr int EST_FC_PF = ENS_BLK * EST_FC / TILE, EST_L_PF = ENS_BLK * EST_L / TILE;   // doubles per lane and block
static_assert(EST_FC_PF * TILE == ENS_BLK * EST_FC && EST_L_PF * TILE == ENS_BLK * EST_L,
              "a block of estimator records is a whole number of doubles per lane");
static_assert(EST_FC % 2 == 0 && EST_O_C % 2 == 0 && EST_L % 2 == 0, "rows of F, c and L start on 16 bytes");

// what the EST instances take beside the arguments of every instance (nothing otherwise: the other instances' arguments
// are what they were)
template <bool EST>
struct EnsEst {};
template <>
struct EnsEst<true> {
    const real* fc;        // [opt][T][EST_FC]
    const real* filter;    // [opt][T][EST_L]
    const real* ehat0;     // [opt][6] or NULL
    MpcNoise mz;           // the measurement noise: sigma = rho, on = whether rho draws
    real* xhat_reg;        // tiled C=6 or NULL
    real* meas_out;        // tiled C=6 or NULL
    real* est_stats;       // [tile][EST_NSTAT][64]
};

// ---- actuator limits and rate limits in the loop (aoc_track_ensemble_limited) ---------------------------------------------
// The LIM instances of k_track_ensemble cut the demand v_t = u_opt_t + K_t dx_t to what an actuator delivers: with the range
// [lo, hi] and the slew s = rate * dt per sample (the product formed once on the host), channel r = 0 thrust, 1 moment,
//     a = lo, b = hi at t = 0;   a = (uprev - s > lo) ? uprev - s : lo,   b = (uprev + s < hi) ? uprev + s : hi at t >= 1,
//     u = v < a ? a : (v > b ? b : v),   uprev = u
// — selections only (a NaN demand fails both comparisons and stays NaN; fmin / fmax would drop it), so with infinite limits
// every output has the bits of the instance without limits.  uprev starts as NaN: both comparisons of a and b fail, which IS
// the rule for t = 0 (there is no u_-1), without a branch on t.  u is what the plant, the cost, every statistic, the envelope
// and the histogram see.  A sample is CUT in channel r when v < a || v > b.
// sat[tile][LIM_NSTAT][64]: 0-1 number of cut samples, 2-3 first cut sample (T if none), 4-5 max_t |v - u| (a NaN sticks).
// cnt (may be NULL): per sample and channel the number of members of the tile that count on the envelope's terms and are
// cut — a ballot and a population count, kept by lane 2 (t % ENS_BLK) + r and written as the tile's partial
// cnt[tile][t][2] once per block of stages (128 contiguous bytes); k_sat_fold adds the tiles of an optimum.
constexpr int LIM_NSTAT = 6;    // AOC_SAT_NSTAT
static_assert(2 * ENS_BLK <= TILE, "one lane per sample and channel of a block of stages");

// what the LIM instances take beside the arguments of every instance (nothing otherwise)
template <bool LIM>
struct EnsLim {};
template <>
struct EnsLim<true> {
    real lo[2], hi[2], s[2];   // s = rate * dt
    real* sat;                 // [tile][LIM_NSTAT][64]
    int* cnt;                  // [tile][T][2] or NULL
};

// ---- limits in the loop of the estimator (aoc_track_ensemble_lqg_limited) -------------------------------------------------
// The EST && LIM instances cut the demand v_t = u_opt_t + K_t e^+_t as the LIM instances do.  The estimator's prediction
// F_t e^+_t + c_t, F = A + B K, assumes the plant received v_t; one that is told the applied input u_t adds what the plant
// got beside it, B_t (u_t - v_t).  B_t has the entries (2,0), (5,0) and (4,1): with g = u - v,
//     e^-[2] += b20 g[0],   e^-[5] += b50 g[0],   e^-[4] += b41 g[1]       (a product and an addition each, two roundings)
// where est_input says APPLIED and the sample is cut in at least one channel — a selection, so a sample that is not cut (and
// every sample under infinite limits, or with est_input = DEMANDED) keeps the bits of the EST instance, a -0.0 included.
// b20 and b50 depend on the optimum: k_cov_stage<true, true> (covariance.inc) writes them where the record's copy of K
// starts (EST_O_B), which the estimator stages through LDS anyway and never reads; b41 is the model's.
constexpr int EST_O_B = 42;     // where b20, b50 lie in a record of k_cov_stage<true, true> (COV_O_K, asserted in lqg.inc)

// what the EST && LIM instances take beside EnsEst and EnsLim (nothing otherwise: those two keep their layout)
template <bool ON>
struct EnsEstLim {};
template <>
struct EnsEstLim<true> {
    int applied;           // est_input == AOC_EST_INPUT_APPLIED
};

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
// ENV: also the per-tile envelope records part[tile][t][ENV_NREC] (above); every other output keeps its bits.
// HIST: also the per-tile byte counts part[tile][t][HIST_NCH][HIST_NBIN] under `bins` (above); never together with ENV.
// EST: the input is fed back from the estimate of `est` (above) instead of the true deviation; never with ENV or HIST.
// LIM: the input is cut to the limits of `lim` (above), with sat and the cut counts.
// EST && LIM: the estimate's demand is cut, and the prediction is told the applied input where `esl` says so (above).
template <bool WRITE, bool NOISE, typename XO, bool DIAG, bool ENV = false, bool HIST = false, bool EST = false,
          bool LIM = false>
__global__ __launch_bounds__(TILE) void k_track_ensemble(KConst kc, int tiles_per_opt, const real* __restrict__ nominal,
                                                         const real* __restrict__ x0, MpcNoise nz, XO* __restrict__ x_reg,
                                                         real* __restrict__ u_reg, real* __restrict__ dist_out,
                                                         real* __restrict__ stats, int* __restrict__ status,
                                                         real* __restrict__ part = nullptr,
                                                         const real* __restrict__ bins = nullptr, EnsEst<EST> est = {},
                                                         EnsLim<LIM> lim = {}, EnsEstLim<EST && LIM> esl = {}) {
#pragma clang fp contract(off)
    static_assert(!(ENV && HIST), "the bins come from an envelope call: the two are never one instance");
    static_assert(!(EST && (ENV || HIST)), "the estimator instances reduce nothing over the members");
    __shared__ __attribute__((aligned(16))) real sh[2][ENS_BLK * ENS_REC];
    __shared__ __attribute__((aligned(16))) real ev[ENV ? ENV_S * ENV_ROWS * ENV_LD : 2];
    __shared__ __attribute__((aligned(16))) real hb[HIST ? 2 * ENS_BLK * HIST_REC : 2];
    __shared__ __attribute__((aligned(16))) unsigned hc[HIST ? HIST_S * HIST_DW : 4];
    __shared__ __attribute__((aligned(16))) real ef[EST ? ENS_BLK * EST_FC : 2];
    __shared__ __attribute__((aligned(16))) real el[EST ? ENS_BLK * EST_L : 2];
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
    real xs[6], xn[6], cur[ENS_REC], q[6], r[2], pf[ENS_PF], hpf[HIST ? HIST_PF : 1];
    const real* __restrict__ bin = HIST ? bins + (size_t)(tile / tiles_per_opt) * T * HIST_REC : nullptr;   // wave-uniform
    const size_t nbin = (size_t)T * HIST_REC;
    real eh[6], se[6];
    unsigned long long me[6] = {0, 0, 0, 0, 0, 0};
    const size_t nfc = (size_t)T * EST_FC, nfl = (size_t)T * EST_L;
    // block b of the nominal = records b*ENS_BLK + 1 .. (b+1)*ENS_BLK (what the stages b*ENS_BLK .. read AHEAD), one
    // coalesced load of ENS_PF doubles per lane; indices beyond the last record are clamped onto it
    auto fetch = [&](int b) {
#pragma unroll
        for (int i = 0; i < ENS_PF; i++) {
            const size_t e = ((size_t)b * ENS_BLK + 1) * ENS_REC + i * TILE + lane;
            pf[i] = nom[e < nrec ? e : nrec - 1];
        }
        if (HIST) {   // block b of the bins = records b*ENS_BLK .. (b+1)*ENS_BLK - 1, clamped likewise
#pragma unroll
            for (int i = 0; i < HIST_PF; i++) {
                const size_t e = (size_t)b * ENS_BLK * HIST_REC + i * TILE + lane;
                hpf[i] = bin[e < nbin ? e : nbin - 1];
            }
        }
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int i = 0; i < ENS_PF; i++) sh[b & 1][i * TILE + lane] = pf[i];
        if (HIST) {
#pragma unroll
            for (int i = 0; i < HIST_PF; i++) hb[(b & 1) * ENS_BLK * HIST_REC + i * TILE + lane] = hpf[i];
        }
        // block b of F / c and of L = the records b*ENS_BLK .. (b+1)*ENS_BLK - 1 (clamped likewise) replaces block b - 1, HERE,
        // between two blocks of stages and not through registers held over a block — unless no sample up to T-1 is in it
        // (then sample T-1 still reads block b - 1)
        if constexpr (EST) {
            if (b * ENS_BLK <= T - 1) {
                const real* __restrict__ fc = est.fc + (size_t)(tile / tiles_per_opt) * nfc;       // wave-uniform
                const real* __restrict__ fl = est.filter + (size_t)(tile / tiles_per_opt) * nfl;
                real fpf[EST_FC_PF], lpf[EST_L_PF];
#pragma unroll
                for (int i = 0; i < EST_FC_PF; i++) {
                    const size_t e = (size_t)b * ENS_BLK * EST_FC + i * TILE + lane;
                    fpf[i] = fc[e < nfc ? e : nfc - 1];
                }
#pragma unroll
                for (int i = 0; i < EST_L_PF; i++) {
                    const size_t e = (size_t)b * ENS_BLK * EST_L + i * TILE + lane;
                    lpf[i] = fl[e < nfl ? e : nfl - 1];
                }
#pragma unroll
                for (int i = 0; i < EST_FC_PF; i++) ef[i * TILE + lane] = fpf[i];
#pragma unroll
                for (int i = 0; i < EST_L_PF; i++) el[i * TILE + lane] = lpf[i];
            }
        }
        __syncthreads();   // one wavefront: orders the LDS writes before the broadcast reads, costs nothing
    };
    // envelope: what this lane reduces (fixed for the whole kernel) and where its results go
    const bool in_B = tile * TILE + lane < k.B;   // the lanes that replicate member B-1 never count
    const int e_s = lane / ENV_NTASK, e_k = lane - e_s * ENV_NTASK;            // sums: sample slot, task
    const unsigned e_t = env_task(e_k);
    const int e_a = e_t >> 8, e_b = (e_t >> 4) & 15, e_c = e_t & 15;
    const int e_row = (e_s < ENV_S ? e_s : 0) * ENV_ROWS;
    const real2v* __restrict__ pa = (const real2v*)&ev[ENV ? (e_row + (e_a == 6 ? 8 : e_a)) * ENV_LD : 0];
    const real2v* __restrict__ pb = (const real2v*)&ev[ENV ? (e_row + (e_b == 6 ? 8 : e_b)) * ENV_LD : 0];
    const real2v* __restrict__ pc = (const real2v*)&ev[ENV ? (e_row + (e_c == 6 ? 8 : e_c)) * ENV_LD : 0];
    const int e_rb = env_rec(e_a, e_b), e_rc = env_rec(e_a, e_c);
    const int m_s = lane >> 4, m_q = (lane >> 1) & 7, m_h = lane & 1;          // min / max: sample slot, quantity, half
    const real2v* __restrict__ pv = (const real2v*)&ev[ENV ? (m_s * ENV_ROWS + m_q) * ENV_LD + m_h * (TILE / 2) : 0];
    const real2v* __restrict__ pp = (const real2v*)&ev[ENV ? (m_s * ENV_ROWS + 9) * ENV_LD + m_h * (TILE / 2) : 0];
    const int m_rmin = m_q < 6 ? 1 + m_q : 7 + m_q, m_rmax = m_q < 6 ? 7 + m_q : 9 + m_q;
    // sample t of this member into slot t % ENV_S
    auto env_put = [&](int t, const real dx[6], real du0, real du1, bool counts) {
        real* __restrict__ row = &ev[(t & (ENV_S - 1)) * ENV_ROWS * ENV_LD + lane];
#pragma unroll
        for (int c = 0; c < 6; c++) row[c * ENV_LD] = counts ? dx[c] : R(0.0);
        row[6 * ENV_LD] = counts ? du0 : R(0.0);
        row[7 * ENV_LD] = counts ? du1 : R(0.0);
        row[8 * ENV_LD] = counts ? R(1.0) : R(0.0);
        row[9 * ENV_LD] = counts ? R(0.0) : (real)__builtin_inf();
    };
    // the samples tb .. tb + ns - 1 (slots 0 .. ns-1) over the 64 members of the tile
    auto env_reduce = [&](int tb, int ns) {
        __syncthreads();   // one wavefront: the rows are written
        real s1 = R(0.0), s2 = R(0.0);
#pragma nounroll   // sixteen members' loads in flight (96 VGPRs): more would not fit beside the state of the stage
        for (int m0 = 0; m0 < TILE / 2; m0 += 8) {
#pragma unroll
            for (int m = 0; m < 8; m++) {   // members 2 (m0 + m) and 2 (m0 + m) + 1, in that order
                const real2v a = pa[m0 + m], b = pb[m0 + m], c = pc[m0 + m];
                s1 = __builtin_fma(a.y, b.y, __builtin_fma(a.x, b.x, s1));
                s2 = __builtin_fma(a.y, c.y, __builtin_fma(a.x, c.x, s2));
            }
        }
        real mn = (real)__builtin_inf(), mxv = -(real)__builtin_inf();
#pragma nounroll
        for (int m0 = 0; m0 < TILE / 4; m0 += 8) {
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const real2v v = pv[m0 + m], pen = pp[m0 + m];
                mn = __builtin_fmin(__builtin_fmin(mn, v.x + pen.x), v.y + pen.y);
                mxv = __builtin_fmax(__builtin_fmax(mxv, v.x - pen.x), v.y - pen.y);
            }
        }
        mn = __builtin_fmin(mn, __shfl_xor(mn, 1));
        mxv = __builtin_fmax(mxv, __shfl_xor(mxv, 1));
        if (m_q >= 6 && tb + m_s == T - 1) {   // no input at the last sample: the empty set
            mn = (real)__builtin_inf();
            mxv = -(real)__builtin_inf();
        }
        real* __restrict__ po = part + ((size_t)tile * T + tb) * ENV_NREC;
        if (lane < ENV_S * ENV_NTASK && e_s < ns) {
            po[e_s * ENV_NREC + e_rb] = s1;
            po[e_s * ENV_NREC + e_rc] = s2;
        }
        if (m_h == 0 && m_s < ns) {
            po[m_s * ENV_NREC + m_rmin] = mn;
            po[m_s * ENV_NREC + m_rmax] = mxv;
        }
        __syncthreads();   // the rows are read before the next samples overwrite them
    };
    // histogram: sample t of this member into slot t % HIST_S: one returnless LDS add per channel (nc of them: sample T-1
    // has no input).  A member that does not count adds 0, wherever its (possibly NaN) values point.
    auto hist_put = [&](int t, const real dx[6], real du0, real du1, bool counts, int nc) {
        const real2v* __restrict__ lw = (const real2v*)&hb[((t / ENS_BLK) & 1) * ENS_BLK * HIST_REC + (t % ENS_BLK) * HIST_REC];
        unsigned* __restrict__ slot = &hc[(t & (HIST_S - 1)) * HIST_DW];
#pragma unroll
        for (int c = 0; c < HIST_NCH; c++) {
            if (c >= nc) break;
            const real v = c < 6 ? dx[c] : (c == 6 ? du0 : du1);
            const real2v b = lw[c];                       // (lo, inv_w): every lane the same address
            const real d = v - b.x, s = d * b.y;          // two roundings (contraction is off)
            const int k = s >= R(63.0) ? 63 : (s >= R(1.0) ? (int)s : 0);   // NaN: both comparisons fail, bin 0
            __hip_atomic_fetch_add(&slot[c * (HIST_NBIN / 4) + (k >> 2)], counts ? 1u << ((k & 3) * 8) : 0u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    // the samples tb .. tb + ns - 1 (slots 0 .. ns-1) of the tile go out as they lie, and the counters start again from 0
    auto hist_drain = [&](int tb, int ns) {
        __syncthreads();   // one wavefront: the adds have landed
        uint4* __restrict__ po = (uint4*)((unsigned*)part + ((size_t)tile * T + tb) * HIST_DW);
        uint4* __restrict__ pc = (uint4*)hc;
#pragma unroll
        for (int i = 0; i < HIST_DRAIN; i++) {
            const int e = i * TILE + lane;                // 16-byte piece e: sample slot e / (HIST_DW / 4)
            const uint4 v = pc[e];
            if (e < ns * (HIST_DW / 4)) po[e] = v;
            pc[e] = make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();   // cleared before the next samples add
    };
    if (HIST) {
        uint4* __restrict__ pc = (uint4*)hc;
#pragma unroll
        for (int i = 0; i < HIST_DRAIN; i++) pc[i * TILE + lane] = make_uint4(0u, 0u, 0u, 0u);
    }
    // estimator: sample t of this member: the measurement of dx, e^+ = e^- + L_t (y - e^-) into ep, the error statistics,
    // and x_opt_t + e^+ (xo = the record of the nominal) and v_t for a checker
    auto est_update = [&](int t, const real dx[6], const real* xo, real ep[6]) {
        if constexpr (EST) {
            __builtin_amdgcn_sched_barrier(0);   // the reads of L stay here (they are not worth 72 registers held earlier)
            real v[6], nu[6];
#pragma unroll
            for (int c = 0; c < 6; c++) v[c] = R(0.0);
            if (NOISE && est.mz.on) {
                MpcNoise mt = est.mz;
                mt.step = est.mz.step + (unsigned)t;
                double dn[6];
                mpc_noise_draw(mt, est.mz.first + (unsigned)member, dn, 1u);
#pragma unroll
                for (int c = 0; c < 6; c++) v[c] = (real)dn[c];
            }
#pragma unroll
            for (int c = 0; c < 6; c++) nu[c] = (dx[c] + v[c]) - eh[c];
            const real2v* __restrict__ Lr = (const real2v*)&el[(t % ENS_BLK) * EST_L];
#pragma unroll
            for (int i = 0; i < 6; i++) {   // every lane the same address: a broadcast
                const real2v l0 = Lr[3 * i], l1 = Lr[3 * i + 1], l2 = Lr[3 * i + 2];
                real s = __builtin_fma(l0.y, nu[1], __builtin_fma(l0.x, nu[0], R(0.0)));
                s = __builtin_fma(l1.y, nu[3], __builtin_fma(l1.x, nu[2], s));
                s = __builtin_fma(l2.y, nu[5], __builtin_fma(l2.x, nu[4], s));
                ep[i] = eh[i] + s;
                const real e = dx[i] - ep[i];
                ens_absmax(me[i], e);
                se[i] = se[i] + e * e;
                if (WRITE && est.xhat_reg) st_stream(&est.xhat_reg[tix<6>(tile, T, t, i, lane)], xo[i] + ep[i]);
                if (WRITE && est.meas_out) st_stream(&est.meas_out[tix<6>(tile, T, t, i, lane)], v[i]);
            }
        }
    };
    // e^-_{t+1} = F_t e^+_t + c_t
    auto est_predict = [&](int t, const real ep[6]) {
        if constexpr (EST) {
            __builtin_amdgcn_sched_barrier(0);   // likewise the reads of F and c
            const real2v* __restrict__ Fr = (const real2v*)&ef[(t % ENS_BLK) * EST_FC];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const real2v f0 = Fr[3 * i], f1 = Fr[3 * i + 1], f2 = Fr[3 * i + 2], cc = Fr[EST_O_C / 2 + i / 2];
                real s = __builtin_fma(f0.y, ep[1], __builtin_fma(f0.x, ep[0], R(0.0)));
                s = __builtin_fma(f1.y, ep[3], __builtin_fma(f1.x, ep[2], s));
                s = __builtin_fma(f2.y, ep[5], __builtin_fma(f2.x, ep[4], s));
                eh[i] = s + ((i & 1) ? cc.y : cc.x);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if constexpr (EST) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
            eh[c] = est.ehat0 ? est.ehat0[(size_t)(tile / tiles_per_opt) * 6 + c] : R(0.0);
            se[c] = R(0.0);
        }
    }
    unsigned long long mx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    real JJ = R(0.0);
    int flags = 0, first_bad = T;
    // limits: the input of the sample before, the three cut statistics per channel, this lane's count of the block
    real up[2] = {(real)__builtin_nan(""), (real)__builtin_nan("")};
    unsigned long long msat[2] = {0, 0};
    int ncut[2] = {0, 0}, fcut[2] = {T, T}, cacc = 0;
    // the six limits in VGPRs, like the weights above: the SGPRs are full, and uniform values they do not hold are parked in
    // VGPR lanes and fetched with v_readlane in every stage
    real llo[2], lhi[2], ls[2];
    if constexpr (LIM) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            llo[r] = lim.lo[r]; lhi[r] = lim.hi[r]; ls[r] = lim.s[r];
            vpin(llo[r]); vpin(lhi[r]); vpin(ls[r]);
        }
    }
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
        real d[6], ep[6], u0, u1;
        // uu_reg = uu_opt + KK @ (xx_reg - xx_opt)   (lqr_tracking.py:280), summed from 0 in index order; EST: K times the
        // estimate of the deviation instead
#pragma unroll
        for (int c = 0; c < 6; c++) d[c] = xs[c] - cur[c];
        est_update(t, d, cur, ep);
        real a0 = R(0.0), a1 = R(0.0);
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const real fb = EST ? ep[c] : d[c];
            a0 += cur[8 + c] * fb;
            a1 += cur[14 + c] * fb;
        }
        est_predict(t, ep);
        u0 = cur[6] + a0;
        u1 = cur[7] + a1;
        const bool vbad = !(xs[2] > R(0.0)), nonfin = !ens_finite6(xs);
        if (vbad) flags |= AOC_ST_VNONPOS;
        if (nonfin) flags |= AOC_ST_NAN;
        if ((vbad || nonfin) && t < first_bad) first_bad = t;
        if constexpr (LIM) {
            const real v[2] = {u0, u1};
            real u[2];
            bool any_cut = false;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const real dn = up[r] - ls[r], hn = up[r] + ls[r];
                const real a = dn > llo[r] ? dn : llo[r], bb = hn < lhi[r] ? hn : lhi[r];
                const bool cut = v[r] < a || v[r] > bb;
                any_cut = any_cut || cut;
                u[r] = v[r] < a ? a : (v[r] > bb ? bb : v[r]);
                up[r] = u[r];
                ncut[r] += cut ? 1 : 0;
                fcut[r] = cut && t < fcut[r] ? t : fcut[r];
                ens_absmax(msat[r], v[r] - u[r]);
                // counted whether cnt is asked for or not (a compare's mask, two scalar and two vector instructions): a branch
                // here would cut the stage into blocks
                const int n_cut = __popcll(__ballot(cut && in_B && first_bad > t));
                cacc = lane == 2 * i + r ? n_cut : cacc;
            }
            if constexpr (EST) {   // e^-_{t+1} += B_t (u_t - v_t) where the estimator is told the applied input
                const real2v bb = *(const real2v*)&ef[(t % ENS_BLK) * EST_FC + EST_O_B];   // every lane the same address
                const real g0 = u[0] - v[0], g1 = u[1] - v[1];
                const bool told = any_cut && esl.applied != 0;
                const real c2 = eh[2] + bb.x * g0, c5 = eh[5] + bb.y * g0, c4 = eh[4] + k.b41 * g1;
                eh[2] = told ? c2 : eh[2];
                eh[5] = told ? c5 : eh[5];
                eh[4] = told ? c4 : eh[4];
            }
            u0 = u[0];
            u1 = u[1];
        }
#pragma unroll
        for (int c = 0; c < 6; c++) ens_absmax(mx[c], d[c]);
        ens_absmax(mx[6], u0 - cur[6]);
        ens_absmax(mx[7], u1 - cur[7]);
        if (ENV) {
            env_put(t, d, u0 - cur[6], u1 - cur[7], in_B && first_bad > t);
            if ((t & (ENV_S - 1)) == ENV_S - 1) env_reduce(t - (ENV_S - 1), ENV_S);
        }
        if (HIST) {
            hist_put(t, d, u0 - cur[6], u1 - cur[7], in_B && first_bad > t, HIST_NCH);
            if ((t & (HIST_S - 1)) == HIST_S - 1) hist_drain(t - (HIST_S - 1), HIST_S);
        }
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
      if constexpr (LIM) {
          if (lim.cnt) {   // the samples t0 .. t0 + n - 1 <= T-2 of the tile, two counts each
              if (lane < 2 * n) lim.cnt[((size_t)tile * T + t0) * 2 + lane] = cacc;
              cacc = 0;
          }
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
    real epT[6];
    est_update(T - 1, dT, cur, epT);
    const bool nonfin = !ens_finite6(xs);
    if (nonfin) flags |= AOC_ST_NAN;
    if ((nonfin || !(xs[2] > R(0.0))) && T - 1 < first_bad) first_bad = T - 1;
    if (ENV) {
        env_put(T - 1, dT, R(0.0), R(0.0), in_B && first_bad > T - 1);
        env_reduce((T - 1) & ~(ENV_S - 1), ((T - 1) & (ENV_S - 1)) + 1);
    }
    if (HIST) {
        hist_put(T - 1, dT, R(0.0), R(0.0), in_B && first_bad > T - 1, 6);
        hist_drain((T - 1) & ~(HIST_S - 1), ((T - 1) & (HIST_S - 1)) + 1);
    }
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
    if constexpr (LIM) {
        real* __restrict__ sa = lim.sat + (size_t)tile * LIM_NSTAT * TILE + lane;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            sa[r * TILE] = (real)ncut[r];
            sa[(2 + r) * TILE] = (real)fcut[r];
            sa[(4 + r) * TILE] = (real)__longlong_as_double((long long)msat[r]);
        }
    }
    if constexpr (EST) {
        real* __restrict__ eo = est.est_stats + (size_t)tile * EST_NSTAT * TILE + lane;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            eo[c * TILE] = (real)__longlong_as_double((long long)me[c]);
            eo[(6 + c) * TILE] = se[c];
        }
    }
}

// envelope[opt][t][q] from part[tile][t][q]: the tiles of an optimum folded in tile order, one thread per number (a sum for
// q = 0 and q >= 17, a minimum for 1-6 and 13-14, a maximum for 7-12 and 15-16).  No atomics: the order is the tile order.
// (A template like k_track_ensemble: instantiated by the fp64 launch function only.)
constexpr int ENV_FOLD_THREADS = 256;
template <typename = void>
__global__ __launch_bounds__(ENV_FOLD_THREADS) void k_envelope_fold(int n_opt, int T, int ntiles, int tiles_per_opt,
                                                                    const real* __restrict__ part, real* __restrict__ envelope) {
    const size_t per_opt = (size_t)T * ENV_NREC, idx = (size_t)blockIdx.x * ENV_FOLD_THREADS + threadIdx.x;
    if (idx >= (size_t)n_opt * per_opt) return;
    const int opt = (int)(idx / per_opt), q = (int)(idx % ENV_NREC);
    const int first = opt * tiles_per_opt, last = first + tiles_per_opt < ntiles ? first + tiles_per_opt : ntiles;
    const real* __restrict__ src = part + (size_t)first * per_opt + (idx - (size_t)opt * per_opt);
    const int kind = (q == 0 || q >= 17) ? 0 : ((q <= 6 || q == 13 || q == 14) ? 1 : 2);
    real acc = kind == 0 ? R(0.0) : (kind == 1 ? (real)__builtin_inf() : -(real)__builtin_inf());
    int i = first;
    for (; i + 16 <= last; i += 16) {   // sixteen loads in flight, folded in order
        real v[16];
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = src[(size_t)j * per_opt];
#pragma unroll
        for (int j = 0; j < 16; j++) acc = kind == 0 ? acc + v[j] : (kind == 1 ? __builtin_fmin(acc, v[j]) : __builtin_fmax(acc, v[j]));
        src += 16 * per_opt;
    }
    for (; i < last; i++, src += per_opt)
        acc = kind == 0 ? acc + *src : (kind == 1 ? __builtin_fmin(acc, *src) : __builtin_fmax(acc, *src));
    envelope[idx] = acc;
}

// hist[opt][t][c][k] (int32) from part[tile][t][c][k] (bytes): the tiles of an optimum added up, one thread per dword of
// the partial = four bins (coalesced dword loads, sixteen in flight; one 16-byte store).  Integers: any order gives the same.
template <typename = void>
__global__ __launch_bounds__(ENV_FOLD_THREADS) void k_histogram_fold(int n_opt, int T, int ntiles, int tiles_per_opt,
                                                                     const unsigned* __restrict__ part, int* __restrict__ hist) {
    const size_t per_opt = (size_t)T * HIST_DW, idx = (size_t)blockIdx.x * ENV_FOLD_THREADS + threadIdx.x;
    if (idx >= (size_t)n_opt * per_opt) return;
    const int opt = (int)(idx / per_opt);
    const int first = opt * tiles_per_opt, last = first + tiles_per_opt < ntiles ? first + tiles_per_opt : ntiles;
    const unsigned* __restrict__ src = part + (size_t)first * per_opt + (idx - (size_t)opt * per_opt);
    // two bytes at a time in the halves of a dword: a group of sixteen tiles adds at most 16 * 64 to a half
    int acc[4] = {0, 0, 0, 0};
    int i = first;
    for (; i + 16 <= last; i += 16) {
        unsigned v[16], even = 0u, odd = 0u;
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = src[(size_t)j * per_opt];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            even += v[j] & 0x00ff00ffu;
            odd += (v[j] >> 8) & 0x00ff00ffu;
        }
        acc[0] += (int)(even & 0xffffu); acc[2] += (int)(even >> 16);
        acc[1] += (int)(odd & 0xffffu);  acc[3] += (int)(odd >> 16);
        src += 16 * per_opt;
    }
    for (; i < last; i++, src += per_opt) {
        const unsigned v = *src;
        acc[0] += (int)(v & 0xffu); acc[1] += (int)((v >> 8) & 0xffu); acc[2] += (int)((v >> 16) & 0xffu); acc[3] += (int)(v >> 24);
    }
    ((int4*)hist)[idx] = make_int4(acc[0], acc[1], acc[2], acc[3]);
}

// sat_count[opt][t][r] (int32) from cnt[tile][t][r]: the tiles of an optimum added up, one thread per number (sixteen loads
// in flight).  Integers: any order gives the same.  Sample T-1 has no input: 0, and no tile wrote it.
template <typename = void>
__global__ __launch_bounds__(ENV_FOLD_THREADS) void k_sat_fold(int n_opt, int T, int ntiles, int tiles_per_opt,
                                                               const int* __restrict__ cnt, int* __restrict__ sat_count) {
    const size_t per_opt = (size_t)T * 2, idx = (size_t)blockIdx.x * ENV_FOLD_THREADS + threadIdx.x;
    if (idx >= (size_t)n_opt * per_opt) return;
    const int opt = (int)(idx / per_opt);
    const size_t in_opt = idx - (size_t)opt * per_opt;
    const int first = opt * tiles_per_opt, last = first + tiles_per_opt < ntiles ? first + tiles_per_opt : ntiles;
    int acc = 0;
    if (in_opt < per_opt - 2) {
        const int* __restrict__ src = cnt + (size_t)first * per_opt + in_opt;
        int i = first;
        for (; i + 16 <= last; i += 16) {
            int v[16];
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = src[(size_t)j * per_opt];
#pragma unroll
            for (int j = 0; j < 16; j++) acc += v[j];
            src += 16 * per_opt;
        }
        for (; i < last; i++, src += per_opt) acc += *src;
    }
    sat_count[idx] = acc;
}

#ifndef AOC_KERNELS_ONLY
// aoc_ensemble_envelope_scratch_bytes: part[ntiles][T][ENV_NREC]; 0 for a geometry the call refuses anyway
static size_t ensemble_envelope_scratch_bytes(int32_t B, int32_t T, int32_t members_per_opt) {
    if (B < 1 || T < 1 || members_per_opt < TILE || members_per_opt % TILE) return 0;
    return (size_t)((B + TILE - 1) / TILE) * (size_t)T * ENV_NREC * sizeof(double);
}

// aoc_ensemble_histogram_scratch_bytes: part[ntiles][T][HIST_NCH][HIST_NBIN] bytes; 0 for a geometry the call refuses anyway
static size_t ensemble_histogram_scratch_bytes(int32_t B, int32_t T, int32_t members_per_opt) {
    if (B < 1 || T < 1 || members_per_opt < TILE || members_per_opt % TILE) return 0;
    return (size_t)((B + TILE - 1) / TILE) * (size_t)T * HIST_DW * sizeof(unsigned);
}

enum { ENS_PLAIN = 0, ENS_ENVELOPE = 1, ENS_HISTOGRAM = 2 };

// aoc_ensemble_limited_scratch_bytes: what the mode's own call takes, rounded up to 16 bytes, then the cut counts'
// cnt[ntiles][T][2] int32 if sat_count is asked for; 0 for a mode or a geometry the call refuses anyway
static size_t ensemble_limited_scratch_bytes(int32_t mode, int32_t B, int32_t T, int32_t members_per_opt, int32_t with_sat_count) {
    if (mode < ENS_PLAIN || mode > ENS_HISTOGRAM || B < 1 || T < 1 || members_per_opt < TILE || members_per_opt % TILE) return 0;
    const size_t own = mode == ENS_ENVELOPE ? ensemble_envelope_scratch_bytes(B, T, members_per_opt)
                                            : (mode == ENS_HISTOGRAM ? ensemble_histogram_scratch_bytes(B, T, members_per_opt) : 0);
    return ((own + 15) & ~(size_t)15) + (with_sat_count ? (size_t)((B + TILE - 1) / TILE) * (size_t)T * 2 * sizeof(int) : 0);
}

// The refusals every ensemble call shares (aoc_track_ensemble and what builds on it, lqg.inc included), in the order they are
// reported; `missing` names a further argument of the caller's that is NULL and must not be (or is nullptr).
static int ens_check_args(const char* fn, const aoc_problem* p, int32_t n_opt, int32_t members_per_opt, const real* nominal,
                          const real* x0_reg, const aoc_mpc_noise* noise, const void* x_reg, const real* u_reg,
                          const real* stats, const char* missing) {
    if (!p) return einval("%s: aoc_problem is NULL", fn);
    if (!nominal) return einval("%s: nominal is NULL", fn);
    if (!x0_reg) return einval("%s: x0_reg is NULL", fn);
    if (!stats) return einval("%s: stats is NULL", fn);
    if (missing) return einval("%s: %s is NULL", fn, missing);
    if (n_opt < 1) return einval("%s: n_opt = %d (need n_opt >= 1)", fn, n_opt);
    if (members_per_opt < TILE || members_per_opt % TILE)
        return einval("%s: members_per_opt = %d is not a positive multiple of %d", fn, members_per_opt, TILE);
    if (p->T < 3) return einval("%s: T = %d (need T >= 3)", fn, p->T);
    if ((long long)p->B <= (long long)(n_opt - 1) * members_per_opt || (long long)p->B > (long long)n_opt * members_per_opt)
        return einval("%s: B = %d members do not fill n_opt = %d groups of members_per_opt = %d (need %lld < B <= %lld)", fn,
                      p->B, n_opt, members_per_opt, (long long)(n_opt - 1) * members_per_opt, (long long)n_opt * members_per_opt);
    if ((x_reg == nullptr) != (u_reg == nullptr))
        return einval("%s: x_reg and u_reg go together (one of them is NULL)", fn);
    if (p->x_out_f32 && x_reg && noise)
        return einval("%s: float32 state storage (x_out_f32 = 1) cannot hold disturbed states: with noise "
                      "x_reg must be fp64", fn);
    if (p->RRt[1] != p->RRt[2])
        return einval("%s: aoc_problem.RRt is not symmetric (R01 = %g, R10 = %g)", fn, p->RRt[1], p->RRt[2]);
    return AOC_OK;
}

// the kernels' form of the caller's disturbance model (NULL: none, on = 0)
static MpcNoise ens_noise(const aoc_mpc_noise* noise) {
    MpcNoise nz;
    memset(&nz, 0, sizeof nz);
    if (noise) {
        nz.key0 = (unsigned)(noise->seed & 0xffffffffull); nz.key1 = (unsigned)(noise->seed >> 32);
        nz.step = noise->step; nz.first = noise->first;
        for (int c = 0; c < 6; c++) nz.sigma[c] = noise->sigma[c];
        nz.on = 1;
    }
    return nz;
}

// Limits (aoc_track_ensemble_limited): `limited` with limits, sat (neither NULL) and sat_count (may be NULL); scratch is then
// laid out as ensemble_limited_scratch_bytes says and its size query is named in the reasons.
// Body of aoc_track_ensemble, (mode ENS_ENVELOPE: with envelope, scratch, scratch_bytes) of aoc_track_ensemble_envelope and
// (mode ENS_HISTOGRAM: with bins, hist, scratch, scratch_bytes) of aoc_track_ensemble_histogram, fn the name
// of the entry point for the reasons.  A template only so that the kernels it names are instantiated where it is called
// — from the fp64 entry points — and not once more in the float32 namespace.
template <typename = void>
static int api_track_ensemble(const char* fn, int mode, const aoc_problem* p, int32_t n_opt, int32_t members_per_opt,
                              const real* nominal, const real* x0_reg, const aoc_mpc_noise* noise, void* x_reg, real* u_reg,
                              real* dist_out, real* stats, int32_t* status, real* envelope, const real* bins, int32_t* hist,
                              void* scratch, size_t scratch_bytes, bool limited = false,
                              const aoc_actuator_limits* limits = nullptr, real* sat = nullptr, int32_t* sat_count = nullptr) {
    if (mode < ENS_PLAIN || mode > ENS_HISTOGRAM)
        return einval("%s: mode = %d (0 statistics, 1 envelope, 2 histogram)", fn, mode);
    const bool env = mode == ENS_ENVELOPE, hst = mode == ENS_HISTOGRAM;
    const char* missing = limited && !limits ? "limits" : (limited && !sat ? "sat" : nullptr);
    if (!missing) missing = env && !envelope ? "envelope" : (hst && !bins ? "bins" : (hst && !hist ? "hist" : nullptr));
    if (int rc = ens_check_args(fn, p, n_opt, members_per_opt, nominal, x0_reg, noise, x_reg, u_reg, stats, missing)) return rc;
    if (limited) {
        for (int r = 0; r < 2; r++) {
            if (limits->lo[r] != limits->lo[r] || limits->hi[r] != limits->hi[r] || limits->rate[r] != limits->rate[r])
                return einval("%s: limits has a NaN in channel %d (lo = %g, hi = %g, rate = %g; infinite values mean none)", fn, r,
                              limits->lo[r], limits->hi[r], limits->rate[r]);
            if (limits->lo[r] > limits->hi[r])
                return einval("%s: limits.lo[%d] = %g > limits.hi[%d] = %g", fn, r, limits->lo[r], r, limits->hi[r]);
            if (limits->rate[r] <= 0)
                return einval("%s: limits.rate[%d] = %g (need rate > 0; +inf means none)", fn, r, limits->rate[r]);
        }
    }
    const char* query = limited ? "aoc_ensemble_limited_scratch_bytes"
                                : (env ? "aoc_ensemble_envelope_scratch_bytes" : "aoc_ensemble_histogram_scratch_bytes");
    const size_t need = limited ? ensemble_limited_scratch_bytes(mode, p->B, p->T, members_per_opt, sat_count != nullptr)
                                : (env ? ensemble_envelope_scratch_bytes(p->B, p->T, members_per_opt)
                                       : (hst ? ensemble_histogram_scratch_bytes(p->B, p->T, members_per_opt) : 0));
    if (env || hst || need) {
        if (!scratch) return einval("%s: scratch is NULL (need %zu bytes, %s)", fn, need, query);
        if (scratch_bytes < need) return einval("%s: scratch_bytes = %zu, need %zu (%s)", fn, scratch_bytes, need, query);
    }
    if (hst && ((uintptr_t)scratch % 16 || (uintptr_t)hist % 16))
        return einval("%s: scratch and hist must be 16-byte aligned", fn);
    if (limited && sat_count && (uintptr_t)scratch % 4) return einval("%s: scratch must be 4-byte aligned", fn);
    KConst k = make_const(p->model, p->QQt, p->RRt, p->QQT, p->B, p->T);
    const MpcNoise nz = ens_noise(noise);
    hipStream_t st = (hipStream_t)p->stream;
    const int tpo = members_per_opt / TILE;
    const bool write = x_reg || dist_out;
    EnsLim<true> lm;
    int* cnt = nullptr;
    if (limited) {
        for (int r = 0; r < 2; r++) {
            lm.lo[r] = limits->lo[r];
            lm.hi[r] = limits->hi[r];
            lm.s[r] = limits->rate[r] * p->model.dt;   // the slew per sample, formed once, here
        }
        if (sat_count)
            cnt = (int*)((char*)scratch + ensemble_limited_scratch_bytes(mode, p->B, p->T, members_per_opt, 0));
        lm.sat = sat;
        lm.cnt = cnt;
    }
    // the cut counts of the tiles folded into sat_count, behind the kernels of the mode
    auto finish = [&]() -> int {
        if (int rc = check_launch(fn)) return rc;
        if (!cnt) return AOC_OK;
        const size_t total = (size_t)n_opt * p->T * 2;
        hipLaunchKernelGGL(k_sat_fold<>, dim3((unsigned)((total + ENV_FOLD_THREADS - 1) / ENV_FOLD_THREADS)),
                           dim3(ENV_FOLD_THREADS), 0, st, n_opt, p->T, k.ntiles, tpo, (const int*)cnt, sat_count);
        return check_launch(fn);
    };
#define AOC_ENS_LAUNCH(W, N, XO, D)                                                                                     \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo, nominal, x0_reg, nz, \
                       (XO*)x_reg, u_reg, dist_out, stats, status)
#define AOC_ENV_LAUNCH(W, N, XO, D)                                                                                      \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D, true>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo, nominal, x0_reg, \
                       nz, (XO*)x_reg, u_reg, dist_out, stats, status, (real*)scratch)
#define AOC_HIST_LAUNCH(W, N, XO, D)                                                                                            \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D, false, true>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo, nominal, x0_reg, \
                       nz, (XO*)x_reg, u_reg, dist_out, stats, status, (real*)scratch, bins)
#define AOC_LIM_LAUNCH(W, N, XO, D)                                                                                     \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D, false, false, false, true>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo, \
                       nominal, x0_reg, nz, (XO*)x_reg, u_reg, dist_out, stats, status, (real*)nullptr, (const real*)nullptr, \
                       EnsEst<false>{}, lm)
#define AOC_LIM_ENV_LAUNCH(W, N, XO, D)                                                                                 \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D, true, false, false, true>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo, \
                       nominal, x0_reg, nz, (XO*)x_reg, u_reg, dist_out, stats, status, (real*)scratch, (const real*)nullptr, \
                       EnsEst<false>{}, lm)
#define AOC_LIM_HIST_LAUNCH(W, N, XO, D)                                                                                \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D, false, true, false, true>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo, \
                       nominal, x0_reg, nz, (XO*)x_reg, u_reg, dist_out, stats, status, (real*)scratch, bins, EnsEst<false>{}, lm)
#define AOC_ENS_DISPATCH(LAUNCH)                                                                                        \
    do {                                                                                                                \
        if (p->x_out_f32 && x_reg) /* (never with noise, see above) */                                                  \
            AOC_DISPATCH_BOOL(k.diag, D, LAUNCH(true, false, float, D));                                                \
        else                                                                                                            \
            AOC_DISPATCH_BOOL(write, W, AOC_DISPATCH_BOOL(nz.on, N, AOC_DISPATCH_BOOL(k.diag, D, LAUNCH(W, N, double, D)))); \
    } while (0)
    if (mode == ENS_PLAIN) {
        if (limited)
            AOC_ENS_DISPATCH(AOC_LIM_LAUNCH);
        else
            AOC_ENS_DISPATCH(AOC_ENS_LAUNCH);
        return finish();
    }
    if (hst) {
        if (limited)
            AOC_ENS_DISPATCH(AOC_LIM_HIST_LAUNCH);
        else
            AOC_ENS_DISPATCH(AOC_HIST_LAUNCH);
        if (int rc = check_launch(fn)) return rc;
        const size_t total = (size_t)n_opt * p->T * HIST_DW;
        hipLaunchKernelGGL(k_histogram_fold<>, dim3((unsigned)((total + ENV_FOLD_THREADS - 1) / ENV_FOLD_THREADS)),
                           dim3(ENV_FOLD_THREADS), 0, st, n_opt, p->T, k.ntiles, tpo, (const unsigned*)scratch, hist);
        return finish();
    }
    if (limited)
        AOC_ENS_DISPATCH(AOC_LIM_ENV_LAUNCH);
    else
        AOC_ENS_DISPATCH(AOC_ENV_LAUNCH);
    if (int rc = check_launch(fn)) return rc;
    const size_t total = (size_t)n_opt * p->T * ENV_NREC;
    hipLaunchKernelGGL(k_envelope_fold<>, dim3((unsigned)((total + ENV_FOLD_THREADS - 1) / ENV_FOLD_THREADS)),
                       dim3(ENV_FOLD_THREADS), 0, st, n_opt, p->T, k.ntiles, tpo, (const real*)scratch, envelope);
#undef AOC_ENS_DISPATCH
#undef AOC_LIM_HIST_LAUNCH
#undef AOC_LIM_ENV_LAUNCH
#undef AOC_LIM_LAUNCH
#undef AOC_HIST_LAUNCH
#undef AOC_ENV_LAUNCH
#undef AOC_ENS_LAUNCH
    return finish();
}
#endif  // AOC_KERNELS_ONLY

