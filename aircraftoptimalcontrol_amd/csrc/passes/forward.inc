// passes/forward.inc — forward pass (LQR rollout, descent, speculated Armijo candidates) on one wavefront per tile and on the role kernels of small batches.
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// Forward pass (see aoc_forward in include/aoc.h).  NSPEC = number of Armijo candidate steps
// (alpha_0 .. alpha_{NSPEC-1}) whose trial rollouts ride along: the pass is bound by the K~ stream
// from HBM, so a second serial chain in the same lane is nearly free and saves a whole
// latency-bound trial round later.  Operands of the next FW_PF stages are in flight in a register ring.
#ifndef AOC_FW_PF
#define AOC_FW_PF 2
#endif
constexpr int FW_PF = AOC_FW_PF;

// ---------------------------------------------------------------------------------------------
// What the four forward kernels share: the load rings, the LQR stage and its epilogue.  (Further down, behind CandBuf:
// the hand-off records, the rule of how many candidates a tile stores, the Armijo trial stage and its epilogue.)
// The kernels differ in WHERE a value comes from and goes to (registers, LDS, which wavefront), never in how it is
// computed: every expression below exists once, so "bit-identical to each other" holds by construction.
// ---------------------------------------------------------------------------------------------
// Load rings: the operands of stage t into a ring slot.  The index is clamped — priming may ask past the end of a
// short horizon, and the tail re-reads the last stage: a ring turns in EVERY stage, so that every path through a
// stage loop issues the same loads and the compiler keeps count of what is in flight.
// STREAM: the one-wavefront-per-tile kernel marks its streams (ld_stream, ld_stream3); the role kernels load plainly.
template <bool STREAM>
__device__ __forceinline__ void fw_ring_kt(const real* __restrict__ Kt, int tile, int T, int t, int lane, real Kb[14]) {
    const int tc = t < T - 1 ? t : T - 2;
#pragma unroll
    for (int c = 0; c < 7; c++) kt_load<STREAM>(Kt, tile, T, tc, c, lane, Kb[c], Kb[7 + c]);
}
template <bool STREAM, bool WITH_X, typename XT>
__device__ __forceinline__ void fw_ring_xu(const XT* __restrict__ x, const real* __restrict__ u, int tile, int T, int t,
                                           int lane, XT xb[6], real ub[2]) {
    const int tc = t < T - 1 ? t : T - 2;
    if (WITH_X) {
#pragma unroll
        for (int c = 0; c < 6; c++) xb[c] = STREAM ? ld_stream3(&x[tix<6>(tile, T, tc, c, lane)]) : x[tix<6>(tile, T, tc, c, lane)];
    }
#pragma unroll
    for (int c = 0; c < 2; c++) ub[c] = STREAM ? ld_stream3(&u[tix<2>(tile, T, tc, c, lane)]) : u[tix<2>(tile, T, tc, c, lane)];
}

// One stage of the LQR rollout, in the two parts the callers put their own work between (the hand-off of (u, du), the
// nominal point).  du_t = K~_t [1; dx_t]   (optcon.py:759)
__device__ __forceinline__ void fw_lqr_du(const real Kc[14], const real dx[6], real& d0, real& d1) {
    d0 = Kc[0]; d1 = Kc[7];
#pragma unroll
    for (int j = 0; j < 6; j++) { d0 += Kc[1 + j] * dx[j]; d1 += Kc[8 + j] * dx[j]; }
}
// The stage's term of the descent and dx_{t+1} = A dx_t + B du_t (optcon.py:760); l, qn, rn: Jacobians and stage-cost
// gradients at the nominal (x_t, u_t), wherever the caller has them from.
__device__ __forceinline__ void fw_lqr_step(const KConst& k, const Lin& l, const real qn[6], const real rn[2], real d0, real d1,
                                            real dx[6], real& desc) {
    // descent (optcon.py:474-477): sum_t (B_t^T lambda_{t+1} + r_t)^T du_t.  With lambda_t = A_t^T lambda_{t+1} + q_t,
    // lambda_{T-1} = q_f and dx_{t+1} = A_t dx_t + B_t du_t, dx_0 = 0 the sum telescopes to
    // sum_t (q_t^T dx_t + r_t^T du_t) + q_f^T dx_{T-1}, so neither lambda nor g = B^T lambda + r has to
    // travel from the backward pass (agreement with the explicit sum: 1e-13 on the golden cases).
    real a = rn[0] * d0 + rn[1] * d1;
#pragma unroll
    for (int j = 0; j < 6; j++) a += qn[j] * dx[j];
    desc += a;
    real ax[6];
    A_vec(k, l, dx, ax);
    dx[0] = ax[0]; dx[1] = ax[1];
    dx[2] = ax[2] + l.b20 * d0;
    dx[3] = ax[3];
    dx[4] = ax[4] + k.b41 * d1;
    dx[5] = ax[5] + l.b50 * d0;
}

// The end of the LQR rollout: du_{T-1} = 0, the terminal term q_f^T dx_{T-1} of the descent (xT: the nominal x_{T-1},
// rrT: its reference row), the NaN flag.
template <bool DIAG>
__device__ __forceinline__ void fw_lqr_finish(const KConst& k, const real xT[6], const real* __restrict__ rrT,
                                              const real dx[6], real desc, int tile, int lane, real* __restrict__ du_out,
                                              real* __restrict__ descent, int* __restrict__ status) {
    const int T = k.T, b = tile * TILE + lane;
    du_out[tix<2>(tile, T, T - 1, 0, lane)] = R(0.0);
    du_out[tix<2>(tile, T, T - 1, 1, lane)] = R(0.0);
    real qf[6];
    term_cost2<DIAG>(k, xT, rrT, qf);
    real a = R(0.0);
#pragma unroll
    for (int j = 0; j < 6; j++) a += qf[j] * dx[j];
    desc += a;
    descent[b] = desc;
    if (status && (desc != desc || desc - desc != R(0.0))) status[b] |= AOC_ST_NAN;
}

// XRC: the iterate's states are not read but re-computed, x_{t+1} = step(x_t, u_t) from x0 — valid when they ARE that
// rollout (aoc_problem.x_is_rollout: every iterate this library wrote); the sin/cos of the stage are needed for the
// re-linearisation anyway, so it costs one step_state per stage and saves the state stream (24 of 168 B per stage).
template <bool DIAG, bool RPT, int NSPEC, bool XRC, typename XT>
__global__ __launch_bounds__(TILE) void k_forward(KConst k, aoc_params prm, const real* __restrict__ ref,
                                                  const XT* __restrict__ x, const real* __restrict__ u,
                                                  const real* __restrict__ x0, const real* __restrict__ Kt,
                                                  real* __restrict__ du_out, real* __restrict__ descent,
                                                  real* __restrict__ J_trial, int* __restrict__ status) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane, T = k.T;
    const int Bp = k.ntiles * TILE;
    real dx[6], xp[NSPEC][6], q[6], r[2], JJ[NSPEC], alpha[NSPEC], rb[8];
    alpha[0] = prm.stepsize_0;
#pragma unroll
    for (int j = 1; j < NSPEC; j++) alpha[j] = prm.beta * alpha[j - 1];  // optcon.py:270
#pragma unroll
    for (int c = 0; c < 6; c++) {
        dx[c] = R(0.0);  // ltv_LQR is called with x0 = 0 (optcon.py:470)
        const real v = x0[((size_t)tile * 6 + c) * TILE + lane];
#pragma unroll
        for (int j = 0; j < NSPEC; j++) xp[j][c] = v;
    }
#pragma unroll
    for (int j = 0; j < NSPEC; j++) JJ[j] = R(0.0);
    real desc = R(0.0);
    real Kb[FW_PF][14], ub[FW_PF][2], xs[6];
    XT xb[XRC ? 1 : FW_PF][6];
#pragma unroll
    for (int i = 0; i < FW_PF; i++) {
        fw_ring_kt<true>(Kt, tile, T, i, lane, Kb[i]);
        fw_ring_xu<true, !XRC>(x, u, tile, T, i, lane, xb[XRC ? 0 : i], ub[i]);
    }
    load_state(x, x0, tile, T, 0, lane, xs);   // sample 0 is x0 (fp64), see load_state
    for (int t0 = 0; t0 < T - 1; t0 += FW_PF) {
#pragma unroll
      for (int i = 0; i < FW_PF; i++) {
        const int t = t0 + i;
        if (t >= T - 1) break;
        real Kc[14];
#pragma unroll
        for (int c = 0; c < 14; c++) Kc[c] = Kb[i][c];
        if (!XRC && t > 0) {
#pragma unroll
            for (int c = 0; c < 6; c++) xs[c] = (real)xb[i][c];
        }
        const real uc0 = ub[i][0], uc1 = ub[i][1];
        const real* rr = ref_row<RPT>(k, ref, tile, lane, t, rb);
        fw_ring_kt<true>(Kt, tile, T, t + FW_PF, lane, Kb[i]);   // refill this slot
        fw_ring_xu<true, !XRC>(x, u, tile, T, t + FW_PF, lane, xb[XRC ? 0 : i], ub[i]);
        // sin/cos of every chain of the stage first — they depend on nothing but the states the stage starts from — and one
        // fix-up region for huge arguments behind them (see trig_fast): the rest of the stage is one basic block
        SC s = trig_fast(xs[3], xs[5]), s2[NSPEC];
        bool huge = trig_huge(xs[3], xs[5]);
#pragma unroll
        for (int j = 0; j < NSPEC; j++) {
            s2[j] = trig_fast(xp[j][3], xp[j][5]);
            huge = huge || trig_huge(xp[j][3], xp[j][5]);
        }
        if (huge) {
            trig_fix(xs[3], xs[5], s);
#pragma unroll
            for (int j = 0; j < NSPEC; j++) trig_fix(xp[j][3], xp[j][5], s2[j]);
        }
        real d0, d1;
        fw_lqr_du(Kc, dx, d0, d1);
        {
            real qn[6], rn[2];
            stage_cost2<DIAG>(k, xs, uc0, uc1, rr, qn, rn);
            const Lin l = linearise(k, xs, uc0, s);   // A, B re-linearised at the nominal (x_t, u_t)
            fw_lqr_step(k, l, qn, rn, d0, d1, dx, desc);
            if (XRC) {   // the next nominal state, bit for bit what the rollout that produced this iterate stored
                real xn[6];
                step_state(k, xs, uc0, uc1, s, xn);
#pragma unroll
                for (int c = 0; c < 6; c++) xs[c] = xn[c];
            }
        }
        st_stream(&du_out[tix<2>(tile, T, t, 0, lane)], d0);
        st_stream(&du_out[tix<2>(tile, T, t, 1, lane)], d1);
        // Armijo trials alpha_0 .. alpha_{NSPEC-1} (optcon.py:250-264), independent chains
#pragma unroll
        for (int j = 0; j < NSPEC; j++) {
            real u0, u1, xpn[6];
            step_inputs(uc0, uc1, alpha[j], d0, d1, u0, u1);
            JJ[j] += stage_cost2<DIAG>(k, xp[j], u0, u1, rr, q, r);
            step_state(k, xp[j], u0, u1, s2[j], xpn);
#pragma unroll
            for (int c = 0; c < 6; c++) xp[j][c] = xpn[c];
        }
      }
    }
    if (!XRC) load_state(x, x0, tile, T, T - 1, lane, xs);
    fw_lqr_finish<DIAG>(k, xs, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), dx, desc, tile, lane, du_out, descent, status);
#pragma unroll
    for (int j = 0; j < NSPEC; j++) {
        JJ[j] += term_cost2<DIAG>(k, xp[j], ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
        J_trial[(size_t)j * Bp + b] = R(0.5) * JJ[j];  // JJ accumulated twice the cost, see stage_cost2
    }
}

// Small batches: the three chains of the forward pass on 1 + NSPEC wavefronts of one workgroup.  Wavefront 0 runs
// the LQR rollout (K~ stream, du, descent, re-linearisation, dx) and publishes (u_t, du_t) of stage t through LDS;
// wavefront 1 + j runs the Armijo trial alpha_j one stage behind.  Same operations on the same values as
// k_forward, so the results are bit-identical; the stage time is that of the longest chain instead of their sum.
// At most FWS_TPG trials per workgroup, so that every wavefront has a SIMD of its CU to itself.  More trials
// (tiny batches: every Armijo candidate rides along, aoc_default_nspec, and no trial round is needed afterwards)
// go to further workgroups of the same tile (blockIdx.y), each of which repeats the LQR rollout — the K~ stream
// is read again, which costs nothing when the batch is this small; only group 0 writes du and the descent.
constexpr int FWS_TPG = 3;
#ifndef AOC_FWB
#define AOC_FWB 4
#endif
// measured, forward pass in ms at 4096 / 8192 / 16 384 trajectories (tools/variant_small.sh): loads of 2 stages in flight,
// blocks of 4: 0.54 / 0.54 / 0.58; of 2: 0.54 / 0.61 / 0.64; one stage, barrier per stage (round 1): 0.59 / 0.55 / 0.58;
// loads of 4 stages in flight: 0.56 / 0.96 / 0.99 (the ring then costs the second workgroup of a CU its registers)
#ifndef AOC_FWS_PF
#define AOC_FWS_PF 2
#endif
// The forward kernel of small batches must fit two workgroups on a CU (8192+ trajectories): 256 registers per wavefront,
// which the pinned constants would exceed by a few without this bound.
// WPE = wavefronts per SIMD the kernel is compiled for.  2: the bound above.  1 (round 5): launches of at most one workgroup
// per CU (tiles x groups <= 256: 4096 trajectories with every candidate riding along, the receding-horizon share of a GPU)
// never put two of these wavefronts on a SIMD, and with the whole register file (512) to itself the stage loop keeps
// everything in registers: under the bound of 256 it spilt 76-132 bytes per lane to scratch memory (600-750 with dense
// weights), i.e. global-memory traffic inside the longest chain of the pass.
#ifndef AOC_FWS_ATTR
#define AOC_FWS_ATTR(WPE) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
#endif
constexpr int FWB = AOC_FWB;   // stages per hand-off block of k_forward_split (4: 16 KB of LDS per workgroup, eight fit a CU)

// Candidate iterates (small batches whose Armijo candidates ALL ride along in the forward pass): every trial
// wavefront stores the trajectory it rolls out anyway — per stage one 24-byte record (x'_{t+1} as float32, see CAND_REC_BYTES; through round 4: 48 bytes with u'_t: three
// vector stores) — and the flags the update would raise, so that the update of a tile whose trajectories all accepted
// one of them is a copy, parallel over the horizon, instead of one more serial rollout (k_ls_final_split).
// n = 0: nothing is stored.  Record of (candidate j, tile, stage t, lane): rec[((j*ntiles + tile)*T + t)*64 + lane].
// The stores are what the forward pass of these batches pays most for (4096 trajectories: ten candidates are 0.98 GB per
// pass, +0.12 ms), and the deep candidates are rarely the accepted ones: a tile stores only the first
// nstored[tile] = max over its trajectories of the previous iteration's trial count + CAND_MARGIN (at least CAND_MIN, at
// most n; everything when there is no previous iteration) and records that number for the update, which copies a tile
// only if every trajectory accepted a candidate that was stored.
// Round 5: a record holds the float32 STATES only — x'_{t+1}, three coalesced 8-byte planes per stage, 24 bytes instead of
// the 48 of (u'_t as fp64, x' as float32, padding): the inputs u'_t = u_t + alpha_j du_t are two operands and one rounding
// away from what the update reads anyway, and it re-computes them bit for bit (same expression, contraction off).
typedef float cand2 __attribute__((ext_vector_type(2)));
constexpr int CAND_REC_BYTES = 3 * sizeof(cand2);
struct CandBuf { cand2* rec; int* flags; int* nstored; int n; };
// plane h (components 2h, 2h+1) of the record of (candidate j, tile, stage t, lane)
__device__ __forceinline__ size_t cand_ix(int j, int ntiles, int tile, int T, int t, int h, int lane) {
    return ((((size_t)j * ntiles + tile) * T + t) * 3 + h) * TILE + lane;
}
// measured (ms per iteration over iterations 0..9, 4096 trajectories from random / perturbed x0; tools/small_iter_time.py):
// everything stored 0.991 / 0.954, at least 7 and margin 2: 0.941 / 0.927, 6 and 3: 0.946 / 0.921, 5 and 3: 0.973 / 0.909
// (a tile that needs one candidate more than it stored makes the whole update wait for its rollout)
#ifndef AOC_CAND_MARGIN
#define AOC_CAND_MARGIN 2
#endif
#ifndef AOC_CAND_MIN
#define AOC_CAND_MIN 7
#endif
constexpr int CAND_MARGIN = AOC_CAND_MARGIN, CAND_MIN = AOC_CAND_MIN;

static size_t cand_bytes(int32_t B, int32_t T, int n) {
    return (size_t)n * ((size_t)aoc_ntiles(B) * T * TILE * CAND_REC_BYTES + (size_t)aoc_ntiles(B) * TILE * sizeof(int)) +
           (n ? align_up((size_t)aoc_ntiles(B) * sizeof(int), 16) : 0);
}
static CandBuf cand_carve(const void* cand, int32_t B, int32_t T, int n) {
    CandBuf c;
    c.n = cand ? n : 0;
    c.rec = (cand2*)cand;
    c.flags = (int*)(c.rec + (size_t)n * aoc_ntiles(B) * T * TILE * 3);
    c.nstored = c.flags + (size_t)n * aoc_ntiles(B) * TILE;
    return c;
}
// ---------------------------------------------------------------------------------------------
// Hand-off records: what one role of a multi-wavefront forward kernel hands the next through LDS, per stage and lane.  A
// record is a few PLANES, a plane one 16-byte pair per lane; every record names its planes ONCE, and its writer and its
// reader go through its put / get.  The LDS arrays are [buffers][stages of a block][planes][TILE][2]: `rec` below is
// what remains behind the first two indices.
// ---------------------------------------------------------------------------------------------
typedef real FwPlane[TILE][2];
__device__ __forceinline__ void pl_put(FwPlane* rec, int p, int lane, real a, real b) { rec[p][lane][0] = a; rec[p][lane][1] = b; }
__device__ __forceinline__ void pl_get(const FwPlane* rec, int p, int lane, real& a, real& b) { a = rec[p][lane][0]; b = rec[p][lane][1]; }
// six values (a state, l_x) on three planes from p on
__device__ __forceinline__ void pl_put6(FwPlane* rec, int p, int lane, const real v[6]) {
#pragma unroll
    for (int c = 0; c < 6; c++) rec[p + (c >> 1)][lane][c & 1] = v[c];
}
__device__ __forceinline__ void pl_get6(const FwPlane* rec, int p, int lane, real v[6]) {
#pragma unroll
    for (int c = 0; c < 6; c++) v[c] = rec[p + (c >> 1)][lane][c & 1];
}
// the Jacobians of the nominal point (LIN -> LQR of k_forward_lin, LIN-b -> LQR of k_forward_duo): field f of
// track_lin_fields on plane f / 2
struct FwRecLin {
    static constexpr int NP = (TRACK_LIN_NF + 1) / 2;
    static __device__ __forceinline__ void put(FwPlane* rec, int lane, Lin& l) {
        track_lin_fields(l, [&](int f, real& v) { rec[f >> 1][lane][f & 1] = v; });
    }
    static __device__ __forceinline__ void get(const FwPlane* rec, int lane, Lin& l) {
        track_lin_fields(l, [&](int f, real& v) { v = rec[f >> 1][lane][f & 1]; });
    }
};
// the rest of the nominal point (LIN -> LQR of k_forward_lin, LIN-a -> LQR of k_forward_duo): l_x, l_u, u
struct FwRecNom {
    static constexpr int LX = 0, LU = 3, U = 4, NP = 5;
    static __device__ __forceinline__ void put(FwPlane* rec, int lane, const real qn[6], const real rn[2], real u0, real u1) {
        pl_put6(rec, LX, lane, qn);
        pl_put(rec, LU, lane, rn[0], rn[1]);
        pl_put(rec, U, lane, u0, u1);
    }
    static __device__ __forceinline__ void get(const FwPlane* rec, int lane, real qn[6], real rn[2], real& u0, real& u1) {
        pl_get6(rec, LX, lane, qn);
        pl_get(rec, LU, lane, rn[0], rn[1]);
        pl_get(rec, U, lane, u0, u1);
    }
};
// LQR -> trials (all three role kernels): (u0, u1), (du0, du1) of a stage
struct FwRecUdu {
    static constexpr int U = 0, DU = 1, NP = 2;
    static __device__ __forceinline__ void put(FwPlane* rec, int lane, real u0, real u1, real d0, real d1) {
        pl_put(rec, U, lane, u0, u1);
        pl_put(rec, DU, lane, d0, d1);
    }
    static __device__ __forceinline__ void get(const FwPlane* rec, int lane, real& u0, real& u1, real& d0, real& d1) {
        pl_get(rec, U, lane, u0, u1);
        pl_get(rec, DU, lane, d0, d1);
    }
};
// LIN-a -> LIN-b of k_forward_duo, what the second half of the nominal point needs of the first: (V, al), (u0, sin gamma),
// (cos gamma, "either angle is huge" as 1.0 / 0.0)
struct FwRecGam {
    static constexpr int VA = 0, US = 1, CH = 2, NP = 3;
    static __device__ __forceinline__ void put(FwPlane* rec, int lane, real V, real al, real u0, real sg, real cg, bool huge) {
        pl_put(rec, VA, lane, V, al);
        pl_put(rec, US, lane, u0, sg);
        pl_put(rec, CH, lane, cg, huge ? R(1.0) : R(0.0));
    }
    static __device__ __forceinline__ void get(const FwPlane* rec, int lane, real& V, real& al, real& u0, real& sg, real& cg, bool& huge) {
        real h;
        pl_get(rec, VA, lane, V, al);
        pl_get(rec, US, lane, u0, sg);
        pl_get(rec, CH, lane, cg, h);
        huge = h != R(0.0);
    }
};
// chain -> cost of k_forward_duo: x'_t (every sample), u'_t (every stage)
struct FwRecTrial {
    static constexpr int X = 0, U = 3, NP = 4;
    static __device__ __forceinline__ void put_x(FwPlane* rec, int lane, const real x[6]) { pl_put6(rec, X, lane, x); }
    static __device__ __forceinline__ void get_x(const FwPlane* rec, int lane, real x[6]) { pl_get6(rec, X, lane, x); }
    static __device__ __forceinline__ void put_u(FwPlane* rec, int lane, real u0, real u1) { pl_put(rec, U, lane, u0, u1); }
    static __device__ __forceinline__ void get_u(const FwPlane* rec, int lane, real& u0, real& u1) { pl_get(rec, U, lane, u0, u1); }
};

// How many candidates this tile stores (see CandBuf): the same number in every workgroup and role of the tile.
__device__ __forceinline__ int fw_cand_plan(const CandBuf& cb, const aoc_params& prm, const int* __restrict__ hint,
                                            const int* __restrict__ status, int b) {
    int nst = cb.n;
    if (cb.n > 0 && hint) {
        int h = hint[b];
        // a lane that has exhausted a search before (and still iterates: hint >= 1) will do so again — near the optimum
        // the verdicts alternate between "first candidate" and "none" — and a tile that then lacks the step of an
        // exhausted search makes the whole update wait for its rollout: such a tile stores everything
        const bool exh_before = status != nullptr && h >= 1 && (status[b] & AOC_ST_ARMIJO_EXH) != 0;
#pragma unroll
        for (int o = TILE / 2; o > 0; o >>= 1) h = max(h, __shfl_xor(h, o));
        if (h >= 1 && h <= prm.armijo_maxiters && __ballot(exh_before) == 0ull) nst = min(cb.n, max(h + CAND_MARGIN, CAND_MIN));
    }
    return nst;
}

// the record of stage t of a stored candidate: x'_{t+1} as float32 on three planes (crec: the lane's record of stage 0)
__device__ __forceinline__ void cand_store(cand2* __restrict__ crec, int t, const real xpn[6]) {
#pragma unroll
    for (int h = 0; h < 3; h++) {
        cand2 v;
        v.x = (float)xpn[2 * h]; v.y = (float)xpn[2 * h + 1];
        crec[((size_t)t * 3 + h) * TILE] = v;
    }
}

// An Armijo trial as its wavefront carries it: the state chain x', twice the cost so far, the flags the update would raise.
struct FwTrial { real xp[6], JJ; int cflags; };
__device__ __forceinline__ void fw_trial_init(FwTrial& tr, const real* __restrict__ x0, int tile, int lane) {
    load_x0(x0, tile, lane, tr.xp);
    tr.JJ = R(0.0);
    tr.cflags = 0;
}
// Stage t of the trial alpha (optcon.py:250-264): u'_t = u_t + alpha du_t, x'_{t+1} = step(x'_t, u'_t) and, if the tile
// keeps this candidate, its record.  COST: also the stage cost of (x'_t, u'_t) against the reference row rr and the
// V <= 0 flag; without it (the chains of k_forward_duo, whose cost is another wavefront's) rr, tr.JJ and tr.cflags are
// not touched.  up = u'_t goes out only for those chains, which hand it on (FwRecTrial::put_u); split and lin drop it.
template <bool DIAG, bool COST>
__device__ __forceinline__ void fw_trial_stage(const KConst& k, const TrigK<real>& tk, const real* __restrict__ rr, real uc0,
                                               real uc1, real d0, real d1, real alpha, int t, bool keep,
                                               cand2* __restrict__ crec, FwTrial& tr, real up[2]) {
    real xpn[6];
    step_inputs(uc0, uc1, alpha, d0, d1, up[0], up[1]);
    if (COST) {
        real q[6], r[2];
        tr.JJ += stage_cost2<DIAG>(k, tr.xp, up[0], up[1], rr, q, r);
        if (!(tr.xp[2] > R(0.0))) tr.cflags |= AOC_ST_VNONPOS;
    }
    const SC s2 = trig(tr.xp[3], tr.xp[5], tk);
    step_state(k, tr.xp, up[0], up[1], s2, xpn);
    if (keep) cand_store(crec, t, xpn);
#pragma unroll
    for (int c = 0; c < 6; c++) tr.xp[c] = xpn[c];
}
// The end of trial j: J' (JJ: twice the cost, terminal cost included, see stage_cost2) and, for a stored candidate, its flags.
__device__ __forceinline__ void fw_trial_finish(real JJ, int cflags, bool keep, int j, int Bp, int b,
                                                real* __restrict__ J_trial, const CandBuf& cb) {
    J_trial[(size_t)j * Bp + b] = R(0.5) * JJ;
    if (keep) cb.flags[(size_t)j * Bp + b] = cflags;
}

template <bool DIAG, bool RPT, typename XT, int WPE>
__global__ __launch_bounds__((1 + FWS_TPG) * TILE) AOC_FWS_ATTR(WPE) void k_forward_split(KConst kc, aoc_params prm, int nspec, CandBuf cb, const real* __restrict__ ref,
                                                                      const XT* __restrict__ x, const real* __restrict__ u,
                                                                      const real* __restrict__ x0, const real* __restrict__ Kt,
                                                                      real* __restrict__ du_out, real* __restrict__ descent,
                                                                      real* __restrict__ J_trial, int* __restrict__ status,
                                                                      const int* __restrict__ hint) {
    // (u_t, du_t) travel from the LQR wavefront to the trial wavefronts in blocks of FWB stages, one barrier per
    // block: every chain here is a recursion of its own (the trials only need the inputs), so nothing forces a
    // hand-off per stage, and a barrier per stage parks every wavefront for about half of it (SQ counters, EXPERIMENTS.md)
    __shared__ __attribute__((aligned(16))) real sh[2][FWB][FwRecUdu::NP][TILE][2];
    AOC_PINNED_CONSTS(DIAG)
    constexpr int PF = AOC_FWS_PF;   // stages of (K~, x, u) loads the LQR wavefront keeps in flight
    static_assert(FWB % PF == 0, "a block is a whole number of prefetch groups");
    const int nblk = (k.T - 1 + FWB - 1) / FWB;
    const bool lead = blockIdx.y == 0;   // the group that owns the outputs of the LQR rollout
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, b = tile * TILE + lane, T = k.T;
    const int Bp = k.ntiles * TILE;
    real rb[8];
    if (wv == 0) {
        real dx[6];
#pragma unroll
        for (int c = 0; c < 6; c++) dx[c] = R(0.0);  // ltv_LQR is called with x0 = 0 (optcon.py:470)
        real desc = R(0.0);
        real Kb[PF][14], ub[PF][2], x0s[6];
        XT xb[PF][6];
        load_x0(x0, tile, lane, x0s);
#pragma unroll
        for (int i = 0; i < PF; i++) {
            fw_ring_kt<false>(Kt, tile, T, i, lane, Kb[i]);
            fw_ring_xu<false, true>(x, u, tile, T, i, lane, xb[i], ub[i]);
        }
        for (int blk = 0; blk <= nblk; blk++) {   // step blk: block blk here, block blk-1 in the trial wavefronts
          real(*dst)[FwRecUdu::NP][TILE][2] = sh[blk & 1];
#pragma unroll
          for (int h = 0; h < FWB / PF; h++) {
#pragma unroll
          for (int i = 0; i < PF; i++) {
            const int t = blk * FWB + h * PF + i;
            real Kc[14], xs[6];
#pragma unroll
            for (int c = 0; c < 14; c++) Kc[c] = Kb[i][c];
#pragma unroll
            for (int c = 0; c < 6; c++) xs[c] = t == 0 ? x0s[c] : (real)xb[i][c];
            const real uc0 = ring_take(ub[i][0]), uc1 = ring_take(ub[i][1]);
            fw_ring_kt<false>(Kt, tile, T, t + PF, lane, Kb[i]);
            fw_ring_xu<false, true>(x, u, tile, T, t + PF, lane, xb[i], ub[i]);
            if (t < T - 1) {
                real qn[6], rn[2], d0, d1;
                fw_lqr_du(Kc, dx, d0, d1);
                FwRecUdu::put(dst[h * PF + i], lane, uc0, uc1, d0, d1);
                stage_cost2<DIAG>(k, xs, uc0, uc1, ref_row<RPT>(k, ref, tile, lane, t, rb), qn, rn);
                const SC s = trig(xs[3], xs[5], tk);
                const Lin l = linearise(k, xs, uc0, s);
                fw_lqr_step(k, l, qn, rn, d0, d1, dx, desc);
                if (lead) {
                    du_out[tix<2>(tile, T, t, 0, lane)] = d0;
                    du_out[tix<2>(tile, T, t, 1, lane)] = d1;
                }
            }
          }
          }
          __syncthreads();
        }
        if (!lead) return;
        real xT[6];
        load_state(x, x0, tile, T, T - 1, lane, xT);
        fw_lqr_finish<DIAG>(k, xT, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), dx, desc, tile, lane, du_out, descent, status);
    } else {
        const int j = blockIdx.y * FWS_TPG + wv - 1;
        const bool live = j < nspec;   // a spare wavefront of the last group only keeps the barriers company
        real alpha = prm.stepsize_0;
        for (int i = 1; i <= j; i++) alpha = prm.beta * alpha;  // optcon.py:270
        const int nst = fw_cand_plan(cb, prm, hint, status, b);
        if (cb.n > 0 && blockIdx.y == 0 && wv == 1 && lane == 0) cb.nstored[tile] = nst;
        const bool keep = live && j < nst;    // wave-uniform
        cand2* __restrict__ crec = cb.rec + cand_ix(keep ? j : 0, k.ntiles, tile, T, 0, 0, lane);
        FwTrial tr;
        real up[2];
        fw_trial_init(tr, x0, tile, lane);
        for (int blk = 0; blk <= nblk; blk++) {
          if (blk >= 1 && live) {
            real(*src)[FwRecUdu::NP][TILE][2] = sh[(blk - 1) & 1];
#pragma unroll 2
            for (int qi = 0; qi < FWB; qi++) {
                const int t = (blk - 1) * FWB + qi;
                if (t >= T - 1) break;
                real uc0, uc1, d0, d1;
                FwRecUdu::get(src[qi], lane, uc0, uc1, d0, d1);
                fw_trial_stage<DIAG, true>(k, tk, ref_row<RPT>(k, ref, tile, lane, t, rb), uc0, uc1, d0, d1, alpha, t, keep, crec, tr, up);
            }
          }
          __syncthreads();
        }
        if (!live) return;
        real q[6];
        tr.JJ += term_cost2<DIAG>(k, tr.xp, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
        fw_trial_finish(tr.JJ, tr.cflags, keep, j, Bp, b, J_trial, cb);
    }
}

// The forward pass of small batches with the LQR wavefront relieved of everything that does not depend on dx.
// In k_forward_split the LQR wavefront is the chain every stage waits for: besides the recursion proper (du = K~ [1; dx],
// dx+ = A dx + B du, descent) it evaluates the stage-cost gradients, sin/cos and the Jacobians of the NOMINAL point —
// 2200 of the 2230 cycles of a stage, with its 15 loads per stage held to two stages of look-ahead by the 63 vector
// memory operations a wavefront may have in flight.  None of that nominal-point work depends on dx: here a second
// wavefront ("LIN") does it one block of stages ahead (x, u loads; l_x, l_u, Lin through LDS), the LQR wavefront keeps
// only the K~ stream (7 loads per stage, six stages ahead) and ~70 instructions per stage, and the Armijo trial
// wavefronts (FWL_TPG per workgroup, two blocks behind the LIN wavefront) become the longest chain of the stage.
// Same operations on the same values as k_forward / k_forward_split: results bit-identical (tested).
// Step blk of every wavefront: LIN block blk | LQR block blk-1 | trials block blk-2; one barrier per step, nblk + 2 steps.
constexpr int FWL_TPG = 2;     // trial wavefronts per workgroup (LQR + LIN + 2 trials: one wavefront per SIMD of a CU)
constexpr int FWL_B = 2;       // stages per hand-off block
#ifndef AOC_FWL_PFQ
#define AOC_FWL_PFQ 4
#endif
#ifndef AOC_FWL_PFL
#define AOC_FWL_PFL 6
#endif
constexpr int FWL_PFQ = AOC_FWL_PFQ, FWL_PFL = AOC_FWL_PFL;   // stages of loads in flight: LQR (K~: 14 doubles per stage), LIN (x, u); multiples of FWL_B
constexpr int FWL_LIN = 0, FWL_NOM = FwRecLin::NP, FWL_NP = FWL_NOM + FwRecNom::NP;   // LIN -> LQR per stage: the Jacobians, then l_x, l_u, u
template <bool DIAG, bool RPT, typename XT, int WPE>
__global__ __launch_bounds__((2 + FWL_TPG) * TILE) AOC_FWS_ATTR(WPE) void k_forward_lin(KConst kc, aoc_params prm, int nspec, CandBuf cb, const real* __restrict__ ref,
                                                                    const XT* __restrict__ x, const real* __restrict__ u,
                                                                    const real* __restrict__ x0, const real* __restrict__ Kt,
                                                                    real* __restrict__ du_out, real* __restrict__ descent,
                                                                    real* __restrict__ J_trial, int* __restrict__ status,
                                                                    const int* __restrict__ hint) {
    static_assert(FWL_PFQ % FWL_B == 0 && FWL_PFL % FWL_B == 0, "the load rings turn a whole number of blocks");
    __shared__ __attribute__((aligned(16))) real shL[2][FWL_B][FWL_NP][TILE][2];         // LIN -> LQR
    __shared__ __attribute__((aligned(16))) real sh[2][FWL_B][FwRecUdu::NP][TILE][2];    // LQR -> trials
    AOC_PINNED_CONSTS(DIAG)
    const int T = k.T, nblk = (T - 1 + FWL_B - 1) / FWL_B, nsteps = nblk + 2;
    const bool lead = blockIdx.y == 0;   // the group that owns the outputs of the LQR rollout
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, b = tile * TILE + lane;
    const int Bp = k.ntiles * TILE;
    real rb[8];
    if (wv == 1) {
        // ---- LIN: nominal point of block blk at step blk
        constexpr int SPB = FWL_PFL / FWL_B;   // steps per turn of the ring
        XT xb[FWL_PFL][6];
        real ub[FWL_PFL][2], x0s[6];
        load_x0(x0, tile, lane, x0s);
#pragma unroll
        for (int i = 0; i < FWL_PFL; i++) fw_ring_xu<false, true>(x, u, tile, T, i, lane, xb[i], ub[i]);
        for (int blk0 = 0; blk0 < nsteps; blk0 += SPB) {
#pragma unroll
          for (int s = 0; s < SPB; s++) {
            const int blk = blk0 + s;
            if (blk >= nsteps) break;
            real(*dst)[FWL_NP][TILE][2] = shL[blk & 1];
#pragma unroll
            for (int qi = 0; qi < FWL_B; qi++) {
                const int i = s * FWL_B + qi;           // ring slot of stage t
                const int t = blk * FWL_B + qi;
                real xs[6];
#pragma unroll
                for (int c = 0; c < 6; c++) xs[c] = t == 0 ? x0s[c] : (real)xb[i][c];
                const real uc0 = ring_take(ub[i][0]), uc1 = ring_take(ub[i][1]);
                fw_ring_xu<false, true>(x, u, tile, T, t + FWL_PFL, lane, xb[i], ub[i]);
                if (t < T - 1) {
                    real qn[6], rn[2];
                    stage_cost2<DIAG>(k, xs, uc0, uc1, ref_row<RPT>(k, ref, tile, lane, t, rb), qn, rn);
                    const SC sc = trig(xs[3], xs[5], tk);
                    Lin l = linearise(k, xs, uc0, sc);
                    FwRecLin::put(dst[qi] + FWL_LIN, lane, l);
                    FwRecNom::put(dst[qi] + FWL_NOM, lane, qn, rn, uc0, uc1);
                }
            }
            __syncthreads();
          }
        }
        return;
    }
    if (wv == 0) {
        // ---- LQR: block blk - 1 at step blk
        constexpr int SPB = FWL_PFQ / FWL_B;   // steps per turn of the ring
        real dx[6];
#pragma unroll
        for (int c = 0; c < 6; c++) dx[c] = R(0.0);  // ltv_LQR is called with x0 = 0 (optcon.py:470)
        real desc = R(0.0);
        real Kb[FWL_PFQ][14];
#pragma unroll
        for (int i = 0; i < FWL_PFQ; i++) fw_ring_kt<false>(Kt, tile, T, i, lane, Kb[i]);
        for (int blk0 = 0; blk0 < nsteps; blk0 += SPB) {
#pragma unroll
          for (int s = 0; s < SPB; s++) {
            const int blk = blk0 + s;
            if (blk >= nsteps) break;
            if (blk >= 1 && blk <= nblk) {
                real(*src)[FWL_NP][TILE][2] = shL[(blk - 1) & 1];
                real(*dst)[FwRecUdu::NP][TILE][2] = sh[(blk - 1) & 1];
#pragma unroll
                for (int qi = 0; qi < FWL_B; qi++) {
                    const int i = ((s + SPB - 1) % SPB) * FWL_B + qi;    // ring slot of stage t = (blk - 1) FWL_B + qi
                    const int t = (blk - 1) * FWL_B + qi;
                    real Kc[14];
#pragma unroll
                    for (int c = 0; c < 14; c++) Kc[c] = Kb[i][c];
                    fw_ring_kt<false>(Kt, tile, T, t + FWL_PFQ, lane, Kb[i]);
                    if (t < T - 1) {
                        Lin l;
                        real qn[6], rn[2], uc0, uc1, d0, d1;
                        FwRecLin::get(src[qi] + FWL_LIN, lane, l);
                        FwRecNom::get(src[qi] + FWL_NOM, lane, qn, rn, uc0, uc1);
                        fw_lqr_du(Kc, dx, d0, d1);
                        FwRecUdu::put(dst[qi], lane, uc0, uc1, d0, d1);
                        fw_lqr_step(k, l, qn, rn, d0, d1, dx, desc);
                        if (lead) {
                            du_out[tix<2>(tile, T, t, 0, lane)] = d0;
                            du_out[tix<2>(tile, T, t, 1, lane)] = d1;
                        }
                    }
                }
            }
            __syncthreads();
          }
        }
        if (!lead) return;
        real xT[6];
        load_state(x, x0, tile, T, T - 1, lane, xT);
        fw_lqr_finish<DIAG>(k, xT, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), dx, desc, tile, lane, du_out, descent, status);
        return;
    }
    {
        // ---- Armijo trial alpha_j: block blk - 2 at step blk
        const int j = blockIdx.y * FWL_TPG + wv - 2;
        const bool live = j < nspec;   // a spare wavefront of the last group only keeps the barriers company
        real alpha = prm.stepsize_0;
        for (int i = 1; i <= j; i++) alpha = prm.beta * alpha;  // optcon.py:270
        const int nst = fw_cand_plan(cb, prm, hint, status, b);
        if (cb.n > 0 && blockIdx.y == 0 && wv == 2 && lane == 0) cb.nstored[tile] = nst;
        const bool keep = live && j < nst;    // wave-uniform
        cand2* __restrict__ crec = cb.rec + cand_ix(keep ? j : 0, k.ntiles, tile, T, 0, 0, lane);
        FwTrial tr;
        real up[2];
        fw_trial_init(tr, x0, tile, lane);
        for (int blk = 0; blk < nsteps; blk++) {
          if (blk >= 2 && live) {
            real(*src)[FwRecUdu::NP][TILE][2] = sh[(blk - 2) & 1];
#pragma unroll
            for (int qi = 0; qi < FWL_B; qi++) {
                const int t = (blk - 2) * FWL_B + qi;
                if (t >= T - 1) break;
                real uc0, uc1, d0, d1;
                FwRecUdu::get(src[qi], lane, uc0, uc1, d0, d1);
                fw_trial_stage<DIAG, true>(k, tk, ref_row<RPT>(k, ref, tile, lane, t, rb), uc0, uc1, d0, d1, alpha, t, keep, crec, tr, up);
            }
          }
          __syncthreads();
        }
        if (!live) return;
        real q[6];
        tr.JJ += term_cost2<DIAG>(k, tr.xp, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
        fw_trial_finish(tr.JJ, tr.cflags, keep, j, Bp, b, J_trial, cb);
    }
}

// ---------------------------------------------------------------------------------------------
// The forward pass of TINY batches (round 5; at most one workgroup per CU: tiles x ceil(candidates / 2) <= 256, i.e. the
// receding-horizon share of a GPU and Newton batches up to ~2700 trajectories): the stage cut into SEVEN roles, so that no
// SIMD of the CU has to issue more than ~200 instructions per stage.
// In k_forward_split a stage lasts as long as its longest wavefront: an Armijo trial (~230 instructions: inputs, stage
// cost, two sin/cos pairs, the step, the candidate record) or the LQR wavefront (~250: loads, stage-cost gradients, two
// sin/cos pairs, Jacobians, du, dx, descent) at the ~5.3 cycles a lone wavefront gets per instruction: 0.6 us per stage,
// 0.3 ms per pass, 43 % of a receding-horizon step (profiles/r05_mpc_step_kernel_timeline.txt).  Here, per workgroup
// (seven wavefronts; wavefront i of a workgroup lands on SIMD i mod 4):
//   SIMD 0: chain A (u' = u + alpha du, sin/cos, the step, the record: ~170)
//   SIMD 1: chain B
//   SIMD 2: LIN-a (loads x, u; stage-cost gradients; sin/cos gamma: ~110)     +  LQR (K~ stream, du, dx, descent: ~95)
//   SIMD 3: LIN-b (sin/cos alpha, Jacobians: ~105)                             +  cost (stage cost of A's and B's states: ~90)
// (eight wavefronts are launched; the fifth and the sixth, which would land beside the chains, end at once: S_BARRIER waits
// for the surviving wavefronts of a workgroup only)
// The nominal-point work is the two-producer split of k_backward5, the LQR wavefront that of k_forward_lin, chain | cost
// that of rollout_split; every value is computed by the expressions of k_forward / k_forward_split (same roundings:
// results bit-identical, tested).  Roles hand blocks of FWD_B stages down the pipeline through LDS, ONE barrier per step:
//   step s:  LIN-a block s | LIN-b block s-1 | LQR block s-2 | chains block s-3 | costs block s-4
// (a block counts SAMPLES here, T of them: the chains publish x'_{T-1} as a last sample for the terminal cost).
// Two candidates per workgroup, further candidates in further workgroups of the tile (blockIdx.y), each repeating the
// nominal-point and LQR roles; group 0 owns du and the descent.
// ---------------------------------------------------------------------------------------------
// stages of loads in flight of the two roles with a ring; measured (k_forward_duo of a receding-horizon step, 16 tiles):
// 2: 266 us, 4: 271, 6: 307, 8: 481 (the rings cost registers and moves in the roles that bound the stage)
#ifndef AOC_FWD_PF
#define AOC_FWD_PF AOC_FWD_B
#endif
// measured (k_forward_duo of a receding-horizon step, 16 tiles): blocks of 2 stages 267 us, of 3 stages 257 us — the hand-off
// (a barrier and two LDS round trips per block) is what keeps the stage above the chain's own 0.44 us; 4 would need 212 KB
#ifndef AOC_FWD_B
#define AOC_FWD_B 3
#endif
constexpr int FWD_B = AOC_FWD_B;       // samples per hand-off block (2: 106 KB of LDS; 3: 159 KB of the CU's 160)
constexpr int FWD_PFA = AOC_FWD_PF;     // LIN-a: stages of (x, u) loads in flight (a multiple of FWD_B)
constexpr int FWD_PFQ = AOC_FWD_PF;     // LQR: stages of K~ loads in flight
#ifdef AOC_FWD_SINGLE   // probe build: one candidate per workgroup (the second chain only keeps the barriers company)
constexpr int FWD_CPG = 1;
#else
constexpr int FWD_CPG = 2;              // candidates per workgroup: the launch has ceil(candidates / FWD_CPG) groups per tile
#endif
template <bool DIAG, bool RPT, typename XT>
__global__ __launch_bounds__(8 * TILE) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_forward_duo(
    KConst kc, aoc_params prm, int nspec, CandBuf cb, const real* __restrict__ ref, const XT* __restrict__ x,
    const real* __restrict__ u, const real* __restrict__ x0, const real* __restrict__ Kt, real* __restrict__ du_out,
    real* __restrict__ descent, real* __restrict__ J_trial, int* __restrict__ status, const int* __restrict__ hint) {
    static_assert(FWD_PFA % FWD_B == 0 && FWD_PFQ % FWD_B == 0, "the load rings turn a whole number of blocks");
    __shared__ __attribute__((aligned(16))) real shAB[2][FWD_B][FwRecGam::NP][TILE][2];        // LIN-a -> LIN-b
    __shared__ __attribute__((aligned(16))) real shAQ[3][FWD_B][FwRecNom::NP][TILE][2];        // LIN-a -> LQR (two steps later)
    __shared__ __attribute__((aligned(16))) real shBQ[2][FWD_B][FwRecLin::NP][TILE][2];        // LIN-b -> LQR
    __shared__ __attribute__((aligned(16))) real shQC[2][FWD_B][FwRecUdu::NP][TILE][2];        // LQR -> chains
    __shared__ __attribute__((aligned(16))) real shCJ[2][2][FWD_B][FwRecTrial::NP][TILE][2];   // chain c -> cost c
    // the uniform constants are pinned in VGPRs ROLE BY ROLE (each role what it uses: all of them in every role would not fit
    // beside the load rings; none of them cost the chains 30 % in scalar moves and scalar-load waits, measured)
    KConst k = kc;
    TrigK<real> tk;
    const int T = k.T, nblk = (T + FWD_B - 1) / FWD_B, nsteps = nblk + 4;
    const bool lead = blockIdx.y == 0;
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, b = tile * TILE + lane;
    const int Bp = k.ntiles * TILE;
    real rb[8];
    if (wv == 4 || wv == 5) return;   // their SIMDs belong to the chains (see above); before any barrier
    if (wv == 2) {
        // ---- LIN-a: loads, stage-cost gradients, sin/cos gamma of block s at step s
        if (AOC_PIN) { if (DIAG) pin_weights<DIAG>(k); pin_trig(tk); }   // (dense weights: 76 doubles, more than fit beside the ring)
        constexpr int SPB = FWD_PFA / FWD_B;
        XT xb[FWD_PFA][6];
        real ub[FWD_PFA][2], x0s[6];
        load_x0(x0, tile, lane, x0s);
#pragma unroll
        for (int i = 0; i < FWD_PFA; i++) fw_ring_xu<false, true>(x, u, tile, T, i, lane, xb[i], ub[i]);
        for (int s0 = 0; s0 < nsteps; s0 += SPB) {
#pragma unroll
          for (int ss = 0; ss < SPB; ss++) {
            const int blk = s0 + ss;
            if (blk >= nsteps) break;
            real(*dAB)[FwRecGam::NP][TILE][2] = shAB[blk & 1];
            real(*dAQ)[FwRecNom::NP][TILE][2] = shAQ[blk % 3];
#pragma unroll
            for (int qi = 0; qi < FWD_B; qi++) {
                const int i = ss * FWD_B + qi;           // ring slot of stage t
                const int t = blk * FWD_B + qi;
                real xs[6];
#pragma unroll
                for (int c = 0; c < 6; c++) xs[c] = t == 0 ? x0s[c] : (real)xb[i][c];
                const real uc0 = ring_take(ub[i][0]), uc1 = ring_take(ub[i][1]);
                fw_ring_xu<false, true>(x, u, tile, T, t + FWD_PFA, lane, xb[i], ub[i]);
                if (t < T - 1) {
                    real qn[6], rn[2];
                    stage_cost2<DIAG>(k, xs, uc0, uc1, ref_row<RPT>(k, ref, tile, lane, t, rb), qn, rn);
                    const real ga = xs[5], al = xs[3] - xs[5];
                    const bool huge = trig_huge(xs[3], xs[5]);      // as trig(): either angle huge -> both through the library
                    real sg, cg;
                    sincos_fast(ga, &sg, &cg, tk);
                    if (huge) sincos_lib(ga, &sg, &cg);
                    FwRecGam::put(dAB[qi], lane, xs[2], al, uc0, sg, cg, huge);
                    FwRecNom::put(dAQ[qi], lane, qn, rn, uc0, uc1);
                }
            }
            __syncthreads();
          }
        }
        return;
    }
    if (wv == 3) {
        // ---- LIN-b: sin/cos alpha and the Jacobians of block s - 1 at step s
        if (AOC_PIN) { pin_model(k); pin_trig(tk); }
        for (int s = 0; s < nsteps; s++) {
            const int blk = s - 1;
            if (blk >= 0 && blk < nblk) {
                real(*src)[FwRecGam::NP][TILE][2] = shAB[blk & 1];
                real(*dst)[FwRecLin::NP][TILE][2] = shBQ[blk & 1];
#pragma unroll
                for (int qi = 0; qi < FWD_B; qi++) {
                    const int t = blk * FWD_B + qi;
                    if (t < T - 1) {
                        real V, al, u0;
                        SC sc;
                        bool huge;
                        FwRecGam::get(src[qi], lane, V, al, u0, sc.sg, sc.cg, huge);
                        sincos_fast(al, &sc.sa, &sc.ca, tk);
                        if (huge) sincos_lib(al, &sc.sa, &sc.ca);
                        Lin l = linearise_va(k, V, al, u0, sc);
                        FwRecLin::put(dst[qi], lane, l);
                    }
                }
            }
            __syncthreads();
        }
        return;
    }
    if (wv == 6) {
        // ---- LQR: du = K~ [1; dx], dx+ = A dx + B du, descent of block s - 2 at step s
        constexpr int SPB = FWD_PFQ / FWD_B;
        real dx[6];
#pragma unroll
        for (int c = 0; c < 6; c++) dx[c] = R(0.0);  // ltv_LQR is called with x0 = 0 (optcon.py:470)
        real desc = R(0.0);
        real Kb[FWD_PFQ][14];
#pragma unroll
        for (int i = 0; i < FWD_PFQ; i++) fw_ring_kt<false>(Kt, tile, T, i, lane, Kb[i]);
        // steps 0, 1 have no block for this role; the ring starts turning at step 2 (block 0)
        __syncthreads();
        __syncthreads();
        for (int b0 = 0; b0 < nsteps - 2; b0 += SPB) {
#pragma unroll
          for (int ss = 0; ss < SPB; ss++) {
            const int blk = b0 + ss;
            if (blk >= nsteps - 2) break;
            if (blk < nblk) {
                real(*sBQ)[FwRecLin::NP][TILE][2] = shBQ[blk & 1];
                real(*sAQ)[FwRecNom::NP][TILE][2] = shAQ[blk % 3];
                real(*dst)[FwRecUdu::NP][TILE][2] = shQC[blk & 1];
#pragma unroll
                for (int qi = 0; qi < FWD_B; qi++) {
                    const int i = ss * FWD_B + qi;
                    const int t = blk * FWD_B + qi;
                    real Kc[14];
#pragma unroll
                    for (int c = 0; c < 14; c++) Kc[c] = Kb[i][c];
                    fw_ring_kt<false>(Kt, tile, T, t + FWD_PFQ, lane, Kb[i]);
                    if (t < T - 1) {
                        Lin l;
                        real qn[6], rn[2], uc0, uc1, d0, d1;
                        FwRecLin::get(sBQ[qi], lane, l);
                        FwRecNom::get(sAQ[qi], lane, qn, rn, uc0, uc1);
                        fw_lqr_du(Kc, dx, d0, d1);
                        FwRecUdu::put(dst[qi], lane, uc0, uc1, d0, d1);
                        fw_lqr_step(k, l, qn, rn, d0, d1, dx, desc);
                        if (lead) {
                            du_out[tix<2>(tile, T, t, 0, lane)] = d0;
                            du_out[tix<2>(tile, T, t, 1, lane)] = d1;
                        }
                    }
                }
            }
            __syncthreads();
          }
        }
        if (!lead) return;
        real xT[6];
        load_state(x, x0, tile, T, T - 1, lane, xT);
        fw_lqr_finish<DIAG>(k, xT, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), dx, desc, tile, lane, du_out, descent, status);
        return;
    }
    {
        // ---- Armijo candidates j = FWD_CPG blockIdx.y + c, c = 0, 1: their state chains (wavefronts 0, 1) and their costs (wavefront 7)
        const bool is_chain = wv < 2;
        const int nst = fw_cand_plan(cb, prm, hint, status, b);
        if (cb.n > 0 && blockIdx.y == 0 && wv == 0 && lane == 0) cb.nstored[tile] = nst;
        const int j0 = blockIdx.y * FWD_CPG;
        const bool live1 = FWD_CPG > 1 && j0 + 1 < nspec;   // the spare candidate of the last group only keeps the barriers company
        if (is_chain) {
            const int c = wv, j = j0 + c;
            const bool live = c == 0 ? j < nspec : live1;
            const bool keep = live && j < nst;    // wave-uniform
            real alpha = prm.stepsize_0;
            for (int i = 1; i <= j; i++) alpha = prm.beta * alpha;  // optcon.py:270
            if (AOC_PIN) { pin_model(k); pin_trig(tk); }
            cand2* __restrict__ crec = cb.rec + cand_ix(keep ? j : 0, k.ntiles, tile, T, 0, 0, lane);
            FwTrial tr;
            real up[2];
            fw_trial_init(tr, x0, tile, lane);
            for (int s = 0; s < nsteps; s++) {
                const int blk = s - 3;
                if (blk >= 0 && blk < nblk && live) {
                    real(*src)[FwRecUdu::NP][TILE][2] = shQC[blk & 1];
                    real(*dst)[FwRecTrial::NP][TILE][2] = shCJ[c][blk & 1];
#pragma unroll
                    for (int qi = 0; qi < FWD_B; qi++) {
                        const int t = blk * FWD_B + qi;
                        if (t > T - 1) break;
                        FwRecTrial::put_x(dst[qi], lane, tr.xp);    // x'_t, for the cost wavefront
                        if (t == T - 1) break;                      // the last sample: no stage
                        real uc0, uc1, d0, d1;
                        FwRecUdu::get(src[qi], lane, uc0, uc1, d0, d1);
                        fw_trial_stage<DIAG, false>(k, tk, nullptr, uc0, uc1, d0, d1, alpha, t, keep, crec, tr, up);
                        FwRecTrial::put_u(dst[qi], lane, up[0], up[1]);
                    }
                }
                __syncthreads();
            }
        } else {
            // the cost wavefront: both candidates of the group, one after the other per stage
            if (AOC_PIN && DIAG) pin_weights<DIAG>(k);
            const bool livec[2] = {j0 < nspec, live1};
            real xs[6], q[6], r[2], JJ[2] = {R(0.0), R(0.0)};
            int cflags[2] = {0, 0};
            for (int s = 0; s < nsteps; s++) {
                const int blk = s - 4;
                if (blk >= 0 && blk < nblk) {
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        if (!livec[c]) continue;
                        real(*src)[FwRecTrial::NP][TILE][2] = shCJ[c][blk & 1];
#pragma unroll
                        for (int qi = 0; qi < FWD_B; qi++) {
                            const int t = blk * FWD_B + qi;
                            if (t > T - 1) break;
                            FwRecTrial::get_x(src[qi], lane, xs);
                            if (t == T - 1) {
                                JJ[c] += term_cost2<DIAG>(k, xs, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
                                break;
                            }
                            real u0, u1;
                            FwRecTrial::get_u(src[qi], lane, u0, u1);
                            JJ[c] += stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, t, rb), q, r);
                            if (!(xs[2] > R(0.0))) cflags[c] |= AOC_ST_VNONPOS;
                        }
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int c = 0; c < 2; c++)
                if (livec[c]) fw_trial_finish(JJ[c], cflags[c], j0 + c < nst, j0 + c, Bp, b, J_trial, cb);
        }
    }
}
