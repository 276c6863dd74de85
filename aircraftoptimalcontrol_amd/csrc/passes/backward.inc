// passes/backward.inc — backward pass (costate, quadratisation, Riccati recursion, gains) on one, two, four, five wavefronts per tile; the gradient sweep.
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// Backward pass (see aoc_backward in include/aoc.h).
// The (x,u) loads of the next BW_PF stages are kept in flight in a register ring.
#ifndef AOC_BW_PF
#define AOC_BW_PF 1
#endif
constexpr int BW_PF = AOC_BW_PF;

// One stage of the backward pass is cut in two: everything that depends only on the iterate and on the costate
// (cost gradients, sin/cos, Jacobians, Hessian terms, the costate recursion itself) and the Riccati / gain
// update, which is the serial recursion proper.  BwIn is what crosses the cut.  The single-wavefront kernel runs
// both halves in one lane; the two-wavefront kernel for small batches runs them on two wavefronts of one
// workgroup, one stage apart, through LDS.  `bw_opaque` keeps the compiler from contracting across the cut in
// the single-wavefront kernel, so that both kernels perform the same roundings (results bit-identical).
constexpr int BW_NF_GN = 20, BW_NF_FULL = 27;   // fields of BwIn that travel: Gauss-Newton / full Hessian
struct BwIn {
    Lin l;
    real hq[6], hr[2];
    real dq[6];           // fxx . lambda added to Q at (2,2),(2,3),(2,5),(3,3),(3,5),(5,5)
    real s02, s03, s05;   // fux . lambda, row 0
};
// Two of the Hessian terms are the exact negatives of two others — the model's second derivatives in theta and gamma
// differ by the sign only, (3,5) = -(3,3) and s05 = -s03 (aircraft_simplified.py:346-347, :378-379; the contracted
// expressions of hessian() round identically) — so they do not travel: two doubles fewer alive across the cut, in LDS
// and in the registers of the one-wavefront kernel, whose full-Hessian variant needs every register it can get.

// the twelve state-dependent entries of the Jacobians, as they travel between wavefronts (TRACK_LIN_NF: how many, one more
// than the largest index below — whoever sizes a record by it follows a field added here)
constexpr int TRACK_LIN_NF = 12;
template <typename F>
__device__ __forceinline__ void track_lin_fields(Lin& l, F f) {
    f(0, l.a02); f(1, l.a05); f(2, l.a12); f(3, l.a15); f(4, l.a22); f(5, l.a23); f(6, l.a25);
    f(7, l.a52); f(8, l.a53); f(9, l.a55); f(10, l.b20); f(11, l.b50);
}

template <bool FULL, typename F>
__device__ __forceinline__ void bw_fields(BwIn& b, F f) {
    f(0, b.l.a02); f(1, b.l.a05); f(2, b.l.a12); f(3, b.l.a15); f(4, b.l.a22); f(5, b.l.a23); f(6, b.l.a25);
    f(7, b.l.a52); f(8, b.l.a53); f(9, b.l.a55); f(10, b.l.b20); f(11, b.l.b50);
#pragma unroll
    for (int i = 0; i < 6; i++) f(12 + i, b.hq[i]);
    f(18, b.hr[0]); f(19, b.hr[1]);
    if (FULL) {
#pragma unroll
        for (int i = 0; i < 4; i++) f(20 + i, b.dq[i]);
        f(24, b.dq[5]); f(25, b.s02); f(26, b.s03);
    }
}
// the fields that did not travel (see BwIn)
template <bool FULL>
__device__ __forceinline__ void bw_derive(BwIn& b) {
    if (FULL) { b.dq[4] = -b.dq[3]; b.s05 = -b.s03; }
    else {
#pragma unroll
        for (int i = 0; i < 6; i++) b.dq[i] = R(0.0);
        b.s02 = b.s03 = b.s05 = R(0.0);
    }
}

template <bool DIAG, bool RPT, bool FULL, bool LAM>
__device__ __forceinline__ void bw_produce(const KConst& k, const real* __restrict__ ref, int tile, int lane, int t,
                                           const real xs[6], real u0, real u1, real lam[6], BwIn& o,
                                           const TrigK<real>& tk = TrigK<real>()) {
    real q[6], r[2], rb[8];
    stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, t, rb), q, r);  // q = l_x, r = l_u (optcon.py:436)
    const SC s = trig(xs[3], xs[5], tk);
    o.l = linearise(k, xs, u0, s);
    if (FULL) {  // kk > 8: Q += fxx.lambda, S = fux.lambda (optcon.py:443-446), lambda = lambda_{t+1}
        const Hess h = hessian(k, xs, u0, s, lam);
        o.dq[0] = h.h22; o.dq[1] = h.h23; o.dq[2] = h.h25; o.dq[3] = h.h33; o.dq[4] = h.h35; o.dq[5] = h.h55;
        o.s02 = h.s02; o.s03 = h.s03; o.s05 = h.s05;
    } else {
#pragma unroll
        for (int i = 0; i < 6; i++) o.dq[i] = R(0.0);
        o.s02 = o.s03 = o.s05 = R(0.0);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) o.hq[i] = R(0.5) * q[i];   // optcon.py:673-674 (Q2)
    o.hr[0] = R(0.5) * r[0]; o.hr[1] = R(0.5) * r[1];      // optcon.py:679
    if (LAM) {  // costate: lambda_t = A^T lambda_{t+1} + l_x   (optcon.py:461)
        real al[6];
        At_vec(k, o.l, lam, al);
#pragma unroll
        for (int i = 0; i < 6; i++) lam[i] = al[i] + q[i];
    }
}

// the stage's Q: the weights Qb, with FULL plus the Hessian terms fxx . lambda
template <bool FULL>
__device__ __forceinline__ void bw_stage_q(const BwIn& in, const real Qb[21], real Qs[21]) {
#pragma unroll
    for (int e = 0; e < 21; e++) Qs[e] = Qb[e];
    if (FULL) {
        Qs[sidx(2, 2)] += in.dq[0]; Qs[sidx(2, 3)] += in.dq[1]; Qs[sidx(2, 5)] += in.dq[2];
        Qs[sidx(3, 3)] += in.dq[3]; Qs[sidx(3, 5)] += in.dq[4]; Qs[sidx(5, 5)] += in.dq[5];
    }
}

template <bool FULL, typename Emit>
__device__ __forceinline__ StageFlags bw_consume(const KConst& k, const BwIn& in, real P[21], real p[6],
                                                 const real Qb[21], Emit emit) {
    real Qs[21];
    bw_stage_q<FULL>(in, Qb, Qs);
    return lqr_stage(k, in.l, P, p, Qs, in.s02, in.s03, in.s05, in.hq, in.hr, emit);
}

// the columns COLS (+ affine terms) of a stage: lqr_stage_part on the same Q as bw_consume
template <bool FULL, int COLS, bool AFFINE, typename Emit>
__device__ __forceinline__ StageFlags bw_consume_part(const KConst& k, const BwIn& in, const real P[21], real p[6],
                                                      const real Qb[21], real Pn[21], Emit emit) {
    real Qs[21];
    bw_stage_q<FULL>(in, Qb, Qs);
    return lqr_stage_part<COLS, AFFINE>(k, in.l, P, p, Qs, in.s02, in.s03, in.s05, in.hq, in.hr, Pn, emit);
}

__device__ __forceinline__ void bw_opaque(double& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void bw_opaque(float& v) { asm volatile("" : "+v"(v)); }

// terminal condition (optcon.py:429-432, :688-690, :716): P = Q_T, p = q_f/2, lambda = q_f
template <bool DIAG, bool RPT, typename XT>
__device__ __forceinline__ void bw_terminal(const KConst& k, const real* __restrict__ ref, const XT* __restrict__ x,
                                            const real* __restrict__ x0, int tile, int lane, real P[21], real p[6],
                                            real lam[6], real Qb[21]) {
    const int T = k.T;
    real xs[6], q[6], rb[8];
    load_state(x, x0, tile, T, T - 1, lane, xs);
    term_cost2<DIAG>(k, xs, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
#pragma unroll
    for (int i = 0; i < 6; i++) {
        lam[i] = q[i];
        p[i] = R(0.5) * q[i];
#pragma unroll
        for (int j = i; j < 6; j++) {
            P[sidx(i, j)] = k.QT[i * 6 + j];
            Qb[sidx(i, j)] = k.Q[i * 6 + j];
        }
    }
}

// LAM: carry the costate lambda (needed for the Hessian terms when FULL, or when lambda_0 is asked for).
#ifndef AOC_BW_ATTR
#define AOC_BW_ATTR
#endif
template <bool DIAG, bool RPT, bool FULL, bool LAM, typename XT>
__global__ __launch_bounds__(TILE) AOC_BW_ATTR void k_backward(KConst k, const real* __restrict__ ref,
                                                   const XT* __restrict__ x, const real* __restrict__ u,
                                                   const real* __restrict__ x0, real* __restrict__ Kt,
                                                   real* __restrict__ lmbd0, int* __restrict__ status) {
    static_assert(LAM || !FULL, "the full Hessian needs the costate");
    const int tile = blockIdx.x, lane = threadIdx.x, T = k.T;
    real P[21], p[6], lam[6], Qb[21], xs[6];
    int flags = 0;
    bw_terminal<DIAG, RPT>(k, ref, x, x0, tile, lane, P, p, lam, Qb);
    XT xb[BW_PF][6];  // kept in storage precision: a float32 ring costs half the registers
    real ubuf[BW_PF][2];
#pragma unroll
    for (int i = 0; i < BW_PF; i++) {
        const int tp = T - 2 - i >= 0 ? T - 2 - i : 0;
#pragma unroll
        for (int c = 0; c < 6; c++) xb[i][c] = ld_stream3(&x[tix<6>(tile, T, tp, c, lane)]);
        ubuf[i][0] = ld_stream3(&u[tix<2>(tile, T, tp, 0, lane)]);
        ubuf[i][1] = ld_stream3(&u[tix<2>(tile, T, tp, 1, lane)]);
    }
    // one stage: everything that depends on the iterate and the costate, then the Riccati / gain recursion, K~_t out
    auto stage = [&](int t, const real xs[6], real u0, real u1) {
        BwIn in;
        bw_produce<DIAG, RPT, FULL, LAM>(k, ref, tile, lane, t, xs, u0, u1, lam, in);
        bw_fields<FULL>(in, [](int, real& v) { bw_opaque(v); });
        bw_derive<FULL>(in);
        const StageFlags fl = bw_consume<FULL>(k, in, P, p, Qb, [&](int c, real a, real b) {
            kt_store<true>(Kt, tile, T, t, c, lane, a, b);   // each column of K~_t leaves as soon as it exists
        });
        if (fl.singular) flags |= AOC_ST_SINGULAR;
        if (fl.regularised) flags |= AOC_ST_REGULARISED;
    };
    // Stages T-2 .. 1 take their state from the ring.  Stage 0 is peeled off: its state is x0 (fp64, its own array), and
    // six doubles kept through the whole loop for that one stage are twelve registers the full-Hessian variant does not
    // have (it needs two wavefronts per SIMD to hide its latencies: 256 registers).
    for (int tb = T - 2; tb >= 1; tb -= BW_PF) {
#pragma unroll
      for (int i = 0; i < BW_PF; i++) {
        const int t = tb - i;
        if (t < 1) break;
#pragma unroll
        for (int c = 0; c < 6; c++) xs[c] = (real)xb[i][c];
        const real u0 = ubuf[i][0], u1 = ubuf[i][1];
        {   // refill this slot with stage t - BW_PF (clamped at 0: the head re-reads stage 0)
            const int tn = t - BW_PF >= 0 ? t - BW_PF : 0;
#pragma unroll
            for (int c = 0; c < 6; c++) xb[i][c] = ld_stream3(&x[tix<6>(tile, T, tn, c, lane)]);
            ubuf[i][0] = ld_stream3(&u[tix<2>(tile, T, tn, 0, lane)]);
            ubuf[i][1] = ld_stream3(&u[tix<2>(tile, T, tn, 1, lane)]);
        }
        stage(t, xs, u0, u1);
      }
    }
    {   // stage 0: x0, and the inputs of sample 0 from the ring slot that holds them
        load_x0(x0, tile, lane, xs);
        real u0 = ubuf[0][0], u1 = ubuf[0][1];
#pragma unroll
        for (int i = 1; i < BW_PF; i++)
            if ((T - 2) % BW_PF == i) { u0 = ubuf[i][0]; u1 = ubuf[i][1]; }
        stage(0, xs, u0, u1);
    }
    if (LAM && lmbd0) {
#pragma unroll
        for (int c = 0; c < 6; c++) lmbd0[((size_t)tile * 6 + c) * TILE + lane] = lam[c];
    }
    if (status && flags) status[tile * TILE + lane] |= flags;
}

constexpr int HC_WHY_MAP = 1 << 29, HC_WHY_TRUE = 1 << 28;   // ... and why (diagnostic: tools/hcut_full_stats.py): a stage of a map / of the true recursion
constexpr int HC_DISTRUST = 1 << 30;   // full-Hessian horizon cut (k_bw_hcut<.., FULL>), per-lane flag word, internal: this LANE's result comes from the sequential kernel
constexpr int BWS_PF = 4;   // stages of (x, u) the producer wavefront of the multi-wavefront backward kernels keeps in flight

// Small batches: with fewer wavefronts than SIMDs every pass is bound by the instruction stream of ONE wavefront
// per tile (~1.4 us per stage here).  Two wavefronts per tile: wavefront 0 produces BwIn of stage t-1 while
// wavefront 1 consumes that of stage t (double-buffered in LDS, one barrier per stage); the stage time becomes
// that of the longer half.
template <bool DIAG, bool RPT, bool FULL, bool LAM, typename XT>
__global__ __launch_bounds__(2 * TILE) void k_backward2(KConst kc, const real* __restrict__ ref,
                                                        const XT* __restrict__ x, const real* __restrict__ u,
                                                        const real* __restrict__ x0, real* __restrict__ Kt,
                                                        real* __restrict__ lmbd0, int* __restrict__ status,
                                                        const int* __restrict__ only_tiles, const int* __restrict__ lane_flags) {
    static_assert(LAM || !FULL, "the full Hessian needs the costate");
    constexpr int NF = FULL ? BW_NF_FULL : BW_NF_GN;
    __shared__ __attribute__((aligned(16))) real sh[2][(NF + 1) / 2][TILE][2];   // two fields per lane side by side: 16-byte LDS accesses
    // only_tiles (the full-Hessian horizon cut, k_bw_hcut<.., FULL>): this launch serves the lanes the cut does not trust
    // (lane_flags & HC_DISTRUST).  A tile without such a lane: the cut's flags become the pass's, nothing else to do.  A tile
    // with one: the whole tile runs (the wavefront is the unit of execution), the distrusted lanes COMMIT — gains and flags —
    // the others keep the cut's.
    bool commit = true;
    if (only_tiles) {
        const int f = lane_flags[blockIdx.x * TILE + (threadIdx.x & (TILE - 1))];
        commit = (f & HC_DISTRUST) != 0;
        if (threadIdx.x < TILE && status && !commit && f) atomicOr(&status[blockIdx.x * TILE + threadIdx.x], f);
        if (!only_tiles[blockIdx.x]) return;      // block-uniform
    }
    AOC_PINNED_CONSTS(DIAG)
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), T = k.T;
    const bool producer = threadIdx.x < TILE;   // wave-uniform
    real P[21], p[6], lam[6], Qb[21], xs[6];
    int flags = 0;
    bw_terminal<DIAG, RPT>(k, ref, x, x0, tile, lane, P, p, lam, Qb);
    // the producer keeps the (x, u) loads of BWS_PF stages in flight: with one wavefront per SIMD a stage lasts about as
    // long as a trip to HBM, and a ring of depth one left the pass waiting for memory every stage
    XT xb[BWS_PF][6];
    real ub[BWS_PF][2], x0s[6];
    if (producer) {
        load_x0(x0, tile, lane, x0s);
#pragma unroll
        for (int i = 0; i < BWS_PF; i++) {
            const int ts = T - 2 - i > 0 ? T - 2 - i : 0;
#pragma unroll
            for (int c = 0; c < 6; c++) xb[i][c] = x[tix<6>(tile, T, ts, c, lane)];
            ub[i][0] = u[tix<2>(tile, T, ts, 0, lane)];
            ub[i][1] = u[tix<2>(tile, T, ts, 1, lane)];
        }
    }
    // step j = 0 .. T-1: the producer handles stage tp = T-2-j (j <= T-2), the consumer stage tc = T-1-j (j >= 1)
    // each role runs its own loop (the same number of barriers in both): with the other role's memory operations on the
    // paths of ONE loop the compiler drained every outstanding load at each stage (s_waitcnt vmcnt(0)), and the producer's
    // ring was one stage deep whatever its size
    if (producer) {
        for (int j0 = 0; j0 < T; j0 += BWS_PF) {
#pragma unroll
          for (int i_ = 0; i_ < BWS_PF; i_++) {
            const int j = j0 + i_;
            if (j >= T) break;
            const int tp = T - 2 - j;
            if (tp >= 0) {
#pragma unroll
                for (int c = 0; c < 6; c++) xs[c] = tp == 0 ? x0s[c] : (real)xb[i_][c];
                const real u0 = ring_take(ub[i_][0]), u1 = ring_take(ub[i_][1]);
                const int tn = tp - BWS_PF >= 0 ? tp - BWS_PF : 0;
#pragma unroll
                for (int c = 0; c < 6; c++) xb[i_][c] = x[tix<6>(tile, T, tn, c, lane)];
                ub[i_][0] = u[tix<2>(tile, T, tn, 0, lane)];
                ub[i_][1] = u[tix<2>(tile, T, tn, 1, lane)];
                BwIn in;
                bw_produce<DIAG, RPT, FULL, LAM>(k, ref, tile, lane, tp, xs, u0, u1, lam, in, tk);
                real(*dst)[TILE][2] = sh[j & 1];
                bw_fields<FULL>(in, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            }
            __syncthreads();
          }
        }
    } else {
        for (int j = 0; j < T; j++) {
          const int tc = T - 1 - j;
          if (j >= 1) {
            BwIn in;
            real(*src)[TILE][2] = sh[(j - 1) & 1];
            bw_fields<FULL>(in, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });
            bw_derive<FULL>(in);
            const StageFlags fl = bw_consume<FULL>(k, in, P, p, Qb, [&](int c, real a, real b) {
                if (commit) kt_store<false>(Kt, tile, T, tc, c, lane, a, b);
            });
            if (fl.singular) flags |= AOC_ST_SINGULAR;
            if (fl.regularised) flags |= AOC_ST_REGULARISED;
          }
          __syncthreads();
        }
    }
    if (producer) {
        if (LAM && lmbd0) {
#pragma unroll
            for (int c = 0; c < 6; c++) lmbd0[((size_t)tile * 6 + c) * TILE + lane] = lam[c];
        }
    } else if (status && flags && commit) {
        atomicOr(&status[tile * TILE + lane], flags);
    }
}

// The Riccati / gain half of a stage on three wavefronts (k_backward4): columns {0,1,2}, {3,4} and {5} + affine terms of
// P_t and K~_t (lqr_stage_part).
#define BW4_C0 0x07
#define BW4_C1 0x18
#define BW4_C2 0x20
#define BW4_A0 false
#define BW4_A1 false
#define BW4_A2 true

// Tiny batches, Gauss-Newton iterations.  Four wavefronts per tile, each with a SIMD of its own: ONE producer (everything
// bw_produce does for a stage) and three consumers that share the Riccati / gain half of the stage by columns of P_t and
// K~_t, exchanging their columns of P_t through LDS.  Four, not more: a fifth wavefront (two producers taking the stages
// in turn were tried: 0.53 ms against 0.40 for this kernel at 1024 trajectories) puts two wavefronts on one SIMD and caps
// every wavefront at 256 registers, which the uniform constants pinned in VGPRs (pin_consts) do not fit — and without
// them the stage loops carry s_mov / s_load / v_readlane traffic that a lone wavefront pays for instruction by instruction.
// Same expressions for every entry as bw_produce / lqr_stage: results bit-identical to the other backward kernels.
// Step j: the producer handles stage T-2-j, the consumers stage T-1-j; T steps, one barrier each.
template <bool DIAG, bool RPT, bool FULL, bool LAM, typename XT>
__global__ __launch_bounds__(4 * TILE) void k_backward4(KConst kc, const real* __restrict__ ref,
                                                        const XT* __restrict__ x, const real* __restrict__ u,
                                                        const real* __restrict__ x0, real* __restrict__ Kt,
                                                        real* __restrict__ lmbd0, int* __restrict__ status) {
    static_assert(LAM || !FULL, "the full Hessian needs the costate");
    constexpr int NF = FULL ? BW_NF_FULL : BW_NF_GN;
    // both hand-offs keep two values per lane side by side (16-byte LDS accesses: half the LDS instructions of a step,
    // which three wavefronts issue at the same moment, right after the barrier); P column-major so that the entries a
    // consumer fetches — the columns it does not own — are runs
    __shared__ __attribute__((aligned(16))) real sh[2][(NF + 1) / 2][TILE][2];
    __shared__ __attribute__((aligned(16))) real shP[2][11][TILE][2];
    AOC_PINNED_CONSTS(DIAG)
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, T = k.T;
    const bool producer = wv == 0;   // wave-uniform
    real P[21], p[6], lam[6], Qb[21], xs[6];
    int flags = 0;
    bw_terminal<DIAG, RPT>(k, ref, x, x0, tile, lane, P, p, lam, Qb);   // every wavefront starts from P_{T-1} = Q_T
    XT xb[BWS_PF][6];
    real ub[BWS_PF][2], x0s[6];
    if (producer) {
        load_x0(x0, tile, lane, x0s);
#pragma unroll
        for (int i = 0; i < BWS_PF; i++) {
            const int ts = T - 2 - i > 0 ? T - 2 - i : 0;
#pragma unroll
            for (int c = 0; c < 6; c++) xb[i][c] = x[tix<6>(tile, T, ts, c, lane)];
            ub[i][0] = u[tix<2>(tile, T, ts, 0, lane)];
            ub[i][1] = u[tix<2>(tile, T, ts, 1, lane)];
        }
    }
    // each role runs its own loop (the same number of barriers in both)
    if (producer) {
        for (int j0 = 0; j0 < T; j0 += BWS_PF) {
#pragma unroll
          for (int i_ = 0; i_ < BWS_PF; i_++) {
            const int j = j0 + i_;
            if (j >= T) break;
            const int tp = T - 2 - j;
            if (tp >= 0) {
#pragma unroll
                for (int c = 0; c < 6; c++) xs[c] = tp == 0 ? x0s[c] : (real)xb[i_][c];
                const real u0 = ring_take(ub[i_][0]), u1 = ring_take(ub[i_][1]);
                const int tn = tp - BWS_PF >= 0 ? tp - BWS_PF : 0;
#pragma unroll
                for (int c = 0; c < 6; c++) xb[i_][c] = x[tix<6>(tile, T, tn, c, lane)];
                ub[i_][0] = u[tix<2>(tile, T, tn, 0, lane)];
                ub[i_][1] = u[tix<2>(tile, T, tn, 1, lane)];
                BwIn in;
                bw_produce<DIAG, RPT, FULL, LAM>(k, ref, tile, lane, tp, xs, u0, u1, lam, in, tk);
                real(*dst)[TILE][2] = sh[j & 1];
                bw_fields<FULL>(in, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            }
            __syncthreads();
          }
        }
    } else {
        const int w3 = wv - 1;
        for (int j = 0; j < T; j++) {
          const int tc = T - 1 - j;
          if (j >= 1) {
            BwIn in;
            real Pn[21];
            StageFlags fl;
            real(*src)[TILE][2] = sh[(j - 1) & 1];
            real(*srcP)[TILE][2] = shP[(j - 1) & 1];
            real(*dstP)[TILE][2] = shP[j & 1];
            // one consumer: the fields it needs (q/2, r/2 only enter the affine terms), the columns of P_{tc+1} the other
            // two computed in the previous step, its part of the stage, its columns of P_t and K~_t out
#define BW4_PART(W, COLS, AFF)                                                                   \
            if (w3 == W) {                                                                       \
                bw_fields<FULL>(in, [&](int f, real& v) {                                        \
                    v = (AFF || f < 12 || f >= BW_NF_GN) ? src[f >> 1][lane][f & 1] : R(0.0);    \
                });                                                                              \
                bw_derive<FULL>(in);                                                             \
                if (j >= 2) {                                                                    \
                    _Pragma("unroll") for (int cc = 0; cc < 6; cc++) {                           \
                        if ((COLS >> cc) & 1) continue;                                          \
                        _Pragma("unroll") for (int i = 0; i <= cc; i++) {                        \
                            const int e = cc * (cc + 1) / 2 + i;                                 \
                            P[sidx(i, cc)] = srcP[e >> 1][lane][e & 1];                          \
                        }                                                                        \
                    }                                                                            \
                }                                                                                \
                fl = bw_consume_part<FULL, COLS, AFF>(k, in, P, p, Qb, Pn, [&](int c, real a, real b) { \
                    kt_store<false>(Kt, tile, T, tc, c, lane, a, b);                             \
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
            BW4_PART(0, BW4_C0, BW4_A0)
            BW4_PART(1, BW4_C1, BW4_A1)
            BW4_PART(2, BW4_C2, BW4_A2)
#undef BW4_PART
            if (w3 == 0) {
                if (fl.singular) flags |= AOC_ST_SINGULAR;
                if (fl.regularised) flags |= AOC_ST_REGULARISED;
            }
          }
          __syncthreads();
        }
    }
    if (producer) {
        if (LAM && lmbd0) {
#pragma unroll
            for (int c = 0; c < 6; c++) lmbd0[((size_t)tile * 6 + c) * TILE + lane] = lam[c];
        }
    } else if (wv == 1 && status && flags) {
        atomicOr(&status[tile * TILE + lane], flags);
    }
}

// Five wavefronts per tile (Gauss-Newton iterations of tiny batches).  In k_backward4 the ONE producer is the longest
// chain of the stage: ~310 instructions (loads, cost gradients, two sin/cos pairs, Jacobians, LDS stores) against 186 / 216 /
// 258 for the three column consumers (ISA count, tools/isa_blocks.py), and a lone wavefront pays ~6 cycles for each.  Here
// the producer is two wavefronts, a stage apart: P1 (loads, cost gradients l_x, l_u, sin/cos of gamma) hands V, alpha =
// theta - gamma, u0 and sin/cos gamma to P2 (sin/cos of alpha, Jacobians), which hands the Jacobians to the consumers; the
// affine consumer takes q/2, r/2 straight from P1's buffer, two steps old.  P1 and P2 are the wavefronts 0 and 4 of the
// workgroup — they share a SIMD, ~150 instructions each, and two wavefronts on a SIMD fill the issue slots a lone one leaves
// empty — the consumers keep a SIMD each.  (The five-wavefront kernel of round 2 lost to k_backward4 because its roles
// needed more than the 256 registers two wavefronts on a SIMD leave each; with the gains leaving lqr_stage_part column by
// column the roles need 180.)  Same expressions for every value as bw_produce / lqr_stage_part: bit-identical results.
// Step j = 0..T: P1 stage T-2-j, P2 stage T-1-j, consumers stage T-j; one barrier per step.
// column split of the three consumers (build knobs for A/B: -DAOC_BW5_SPLIT=0 is k_backward4's {0,1,2} | {3,4} | {5} + affine)
#ifndef AOC_BW5_SPLIT
#define AOC_BW5_SPLIT 1
#endif
#if AOC_BW5_SPLIT == 1
#define BW5_C0 0x0F   // columns 0..3
#define BW5_C1 0x10   // column 4 + affine terms
#define BW5_C2 0x20   // column 5
#define BW5_A0 false
#define BW5_A1 true
#define BW5_A2 false
#else
#define BW5_C0 BW4_C0
#define BW5_C1 BW4_C1
#define BW5_C2 BW4_C2
#define BW5_A0 BW4_A0
#define BW5_A1 BW4_A1
#define BW5_A2 BW4_A2
#endif
template <bool DIAG, bool RPT, typename XT>
__global__ __launch_bounds__(5 * TILE) void k_backward5(KConst kc, const real* __restrict__ ref,
                                                        const XT* __restrict__ x, const real* __restrict__ u,
                                                        const real* __restrict__ x0, real* __restrict__ Kt,
                                                        int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real shA[3][7][TILE][2];    // P1 -> P2: (V, al), (u0, sg), (cg, huge); P1 -> affine consumer: q/2 (3 pairs), r/2
    __shared__ __attribute__((aligned(16))) real shB[2][6][TILE][2];    // P2 -> consumers: Lin
    __shared__ __attribute__((aligned(16))) real shP[2][11][TILE][2];   // consumers <-> consumers: the columns of P_t
    AOC_PINNED_CONSTS(DIAG)
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), wv = threadIdx.x >> 6, T = k.T;
    if (wv == 0) {
        // ---- P1
        XT xb[BWS_PF][6];
        real ub[BWS_PF][2], x0s[6], rb[8];
        load_x0(x0, tile, lane, x0s);
#pragma unroll
        for (int i = 0; i < BWS_PF; i++) {
            const int ts = T - 2 - i > 0 ? T - 2 - i : 0;
#pragma unroll
            for (int c = 0; c < 6; c++) xb[i][c] = x[tix<6>(tile, T, ts, c, lane)];
            ub[i][0] = u[tix<2>(tile, T, ts, 0, lane)];
            ub[i][1] = u[tix<2>(tile, T, ts, 1, lane)];
        }
        for (int j0 = 0; j0 <= T; j0 += BWS_PF) {
#pragma unroll
          for (int i_ = 0; i_ < BWS_PF; i_++) {
            const int j = j0 + i_;
            if (j > T) break;
            const int tp = T - 2 - j;
            if (tp >= 0) {
                real xs[6], q[6], r[2];
#pragma unroll
                for (int c = 0; c < 6; c++) xs[c] = tp == 0 ? x0s[c] : (real)xb[i_][c];
                const real u0 = ring_take(ub[i_][0]), u1 = ring_take(ub[i_][1]);
                const int tn = tp - BWS_PF >= 0 ? tp - BWS_PF : 0;
#pragma unroll
                for (int c = 0; c < 6; c++) xb[i_][c] = x[tix<6>(tile, T, tn, c, lane)];
                ub[i_][0] = u[tix<2>(tile, T, tn, 0, lane)];
                ub[i_][1] = u[tix<2>(tile, T, tn, 1, lane)];
                stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, tp, rb), q, r);   // q = l_x, r = l_u (optcon.py:436)
                const real ga = xs[5], al = xs[3] - xs[5];
                const bool huge = trig_huge(xs[3], xs[5]);      // as trig(): either angle huge -> both through the library
                real sg, cg;
                sincos_fast(ga, &sg, &cg, tk);
                if (huge) sincos_lib(ga, &sg, &cg);
                real(*dst)[TILE][2] = shA[j % 3];
                dst[0][lane][0] = xs[2]; dst[0][lane][1] = al;
                dst[1][lane][0] = u0;    dst[1][lane][1] = sg;
                dst[2][lane][0] = cg;    dst[2][lane][1] = huge ? R(1.0) : R(0.0);
#pragma unroll
                for (int c = 0; c < 6; c++) dst[3 + (c >> 1)][lane][c & 1] = R(0.5) * q[c];   // optcon.py:673-674 (Q2)
                dst[6][lane][0] = R(0.5) * r[0]; dst[6][lane][1] = R(0.5) * r[1];              // optcon.py:679
            }
            __syncthreads();
          }
        }
        return;
    }
    if (wv == 4) {
        // ---- P2
        for (int j = 0; j <= T; j++) {
            if (j >= 1 && j <= T - 1) {
                real(*src)[TILE][2] = shA[(j - 1) % 3];
                const real V = src[0][lane][0], al = src[0][lane][1], u0 = src[1][lane][0];
                SC s;
                s.sg = src[1][lane][1]; s.cg = src[2][lane][0];
                const bool huge = src[2][lane][1] != R(0.0);
                sincos_fast(al, &s.sa, &s.ca, tk);
                if (huge) sincos_lib(al, &s.sa, &s.ca);
                Lin l = linearise_va(k, V, al, u0, s);
                real(*dst)[TILE][2] = shB[j & 1];
                track_lin_fields(l, [&](int f, real& v) { dst[f >> 1][lane][f & 1] = v; });
            }
            __syncthreads();
        }
        return;
    }
    // ---- consumers: the columns of P_t and K~_t in three parts (BW5_C*), the affine terms with one of them
    const int w3 = wv - 1;
    real P[21], p[6], lam[6], Qb[21];
    int flags = 0;
    bw_terminal<DIAG, RPT>(k, ref, x, x0, tile, lane, P, p, lam, Qb);   // every consumer starts from P_{T-1} = Q_T
    for (int j = 0; j <= T; j++) {
        const int tc = T - j;
        if (j >= 2) {
            BwIn in;
            real Pn[21];
            StageFlags fl;
            real(*src)[TILE][2] = shB[(j - 1) & 1];
            real(*srcA)[TILE][2] = shA[(j - 2) % 3];
            real(*srcP)[TILE][2] = shP[(j - 1) & 1];
            real(*dstP)[TILE][2] = shP[j & 1];
#define BW5_PART(W, COLS, AFF)                                                                   \
            if (w3 == W) {                                                                       \
                track_lin_fields(in.l, [&](int f, real& v) { v = src[f >> 1][lane][f & 1]; });   \
                _Pragma("unroll") for (int c = 0; c < 6; c++)                                    \
                    in.hq[c] = AFF ? srcA[3 + (c >> 1)][lane][c & 1] : R(0.0);                   \
                in.hr[0] = AFF ? srcA[6][lane][0] : R(0.0);                                      \
                in.hr[1] = AFF ? srcA[6][lane][1] : R(0.0);                                      \
                bw_derive<false>(in);                                                            \
                if (j >= 3) {                                                                    \
                    _Pragma("unroll") for (int cc = 0; cc < 6; cc++) {                           \
                        if ((COLS >> cc) & 1) continue;                                          \
                        _Pragma("unroll") for (int i = 0; i <= cc; i++) {                        \
                            const int e = cc * (cc + 1) / 2 + i;                                 \
                            P[sidx(i, cc)] = srcP[e >> 1][lane][e & 1];                          \
                        }                                                                        \
                    }                                                                            \
                }                                                                                \
                fl = bw_consume_part<false, COLS, AFF>(k, in, P, p, Qb, Pn, [&](int c, real a, real b) { \
                    kt_store<false>(Kt, tile, T, tc, c, lane, a, b);                             \
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
            BW5_PART(0, BW5_C0, BW5_A0)
            BW5_PART(1, BW5_C1, BW5_A1)
            BW5_PART(2, BW5_C2, BW5_A2)
#undef BW5_PART
            if (w3 == 0) {
                if (fl.singular) flags |= AOC_ST_SINGULAR;
                if (fl.regularised) flags |= AOC_ST_REGULARISED;
            }
        }
        __syncthreads();
    }
    if (wv == 1 && status && flags) atomicOr(&status[tile * TILE + lane], flags);
}

// GradientMethod.optimize's direction (optcon.py:101-123): the costate sweep alone,
//   lambda_{T-1} = grad l_T,  du_t = -(B_t^T lambda_{t+1} + l_u),  lambda_t = A_t^T lambda_{t+1} + l_x   (t = T-2 .. 0),
// and slope = -sum_t |du_t|^2: the directional derivative of the cost along du, i.e. what armijo_stepsize takes as
// its `descent` argument (the reference accumulates +sum |du_t|^2 under that name, :123, and prints it).
template <bool DIAG, bool RPT, typename XT>
__global__ __launch_bounds__(TILE) void k_gradient(KConst k, const real* __restrict__ ref, const XT* __restrict__ x,
                                                   const real* __restrict__ u, const real* __restrict__ x0,
                                                   real* __restrict__ du_out, real* __restrict__ slope,
                                                   int* __restrict__ status) {
    const int tile = blockIdx.x, lane = threadIdx.x, T = k.T;
    real lam[6], xs[6], q[6], r[2], rb[8];
    load_state(x, x0, tile, T, T - 1, lane, xs);
    term_cost2<DIAG>(k, xs, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), lam);
    real acc = R(0.0);
    for (int t = T - 2; t >= 0; t--) {
        load_state(x, x0, tile, T, t, lane, xs);
        const real u0 = u[tix<2>(tile, T, t, 0, lane)], u1 = u[tix<2>(tile, T, t, 1, lane)];
        stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, t, rb), q, r);
        const SC s = trig(xs[3], xs[5]);
        const Lin l = linearise(k, xs, u0, s);
        const real d0 = -(l.b20 * lam[2] + l.b50 * lam[5]) - r[0];
        const real d1 = -(k.b41 * lam[4]) - r[1];
        du_out[tix<2>(tile, T, t, 0, lane)] = d0;
        du_out[tix<2>(tile, T, t, 1, lane)] = d1;
        acc += d0 * d0 + d1 * d1;
        real al[6];
        At_vec(k, l, lam, al);
#pragma unroll
        for (int i = 0; i < 6; i++) lam[i] = al[i] + q[i];
    }
    du_out[tix<2>(tile, T, T - 1, 0, lane)] = R(0.0);
    du_out[tix<2>(tile, T, T - 1, 1, lane)] = R(0.0);
    const int b = tile * TILE + lane;
    slope[b] = -acc;
    if (status && (acc != acc || acc - acc != R(0.0))) status[b] |= AOC_ST_NAN;
}

