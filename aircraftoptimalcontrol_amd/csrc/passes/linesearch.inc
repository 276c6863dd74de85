// passes/linesearch.inc — Armijo line search and update: round-based search, work-list search, copying and rolling updates.
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// Armijo back-tracking (optcon.py:243-273) + final update (optcon.py:488-491), batched.
//
// A rollout is a strictly serial chain over T stages and a wavefront issues in order, so one trial
// costs ~T * (a few hundred instructions) of wall time however few trajectories still search, and
// back-tracking inside a tile would cost max-over-64-lanes trials per wavefront (mean trials are
// 1.2-2.2, the max over a tile is 5-8).  So the search runs in rounds over the still-searching
// trajectories only, compacted in tile order over as few wavefronts as possible, and when those are
// fewer than the chip has SIMDs the round evaluates the next K candidate steps of every trajectory
// at once, each (trajectory, step) pair on its own lane: the reference tries steps one by one, the
// first accepted index is the same.
//   k_ls_init  : trial-0 verdicts (J' of aoc_forward) -> bit mask per tile; step table a_r = s0*beta^r
//   k_ls_plan  : (one workgroup) resolve the previous round, prefix-sum the masks, choose K
//   k_ls_trial : cost-only rollouts of (trajectory, a_{r+k}); accept -> atomicMin(first_ok[b], r+k)
//   k_ls_final : resolve the last round; exhausted searches take the never-evaluated
//                s0*beta^maxiters (Q5); every trajectory is rolled out with its step into x_new/u_new
//                (full-tile coalesced stores) and J_new
// A compacted lane gathers its (u, du) elements from its home tile; the work list is in tile order,
// so a wavefront touches about the cache lines a coalesced pass over the same tiles would.
// ---------------------------------------------------------------------------------------------
constexpr int LS_MAX_STEPS = 64;   // armijo_maxiters <= 63
constexpr int LS_NOT_FOUND = 0x7fffffff;
#ifndef AOC_LS_ROUNDS
#define AOC_LS_ROUNDS 4
#endif
constexpr int LS_ROUNDS = AOC_LS_ROUNDS;   // trial rounds launched after the speculative trials of the forward pass

constexpr int LS_WL_IPL = 8;      // work items one trajectory may put on the list of one round
constexpr int LS_WL_ROUNDS = 16;   // rounds the work-list search may need at most (63 candidates, one per lane and item)

struct LsState {
    int r_next;   // first step index not yet evaluated
    int r_start;  // this round evaluates indices r_start .. r_start+K-1
    int K;
    int count;    // trajectories searching in this round
    int nw;       // wavefronts per step index = ceil(count/64)
    int round;    // rounds planned so far
    int scheme;   // 0: round-based search (k_ls_init ...), 1: work-list search (k_ls_init_wl ...): how the update resolves
    int pad;
    real alpha[LS_MAX_STEPS];
};

struct LsScratch {
    unsigned long long* mask;  // [ntiles]  bit l: lane l still searching
    int* prefix;               // [ntiles+1]
    int* first_ok;             // [ntiles*64]
    LsState* st;
    // work-list line search (k_ls_init_wl, k_ls_trial_wl, k_ls_replan)
    int2* items;               // [ntiles*64*LS_WL_IPL]  (trajectory b, first candidate | count << 8)
    int* next_r;               // [ntiles*64]  first candidate index not yet put on a work list
    int* wl_count;             // [2 * LS_WL_ROUNDS]  items on the list of each round; [LS_WL_ROUNDS]: trajectories searching
};

// frozen (aoc_newton_solve only): trajectories that have stopped iterating but still ride along in their tile;
// frozen.orig[b] = index of lane b's trajectory in the caller's batch (-1: padding), frozen.ret[that] != -2
// once it has stopped.  Such a lane takes the step 0 and never searches.
struct LsFrozen { const int* orig; const int* ret; };

__global__ __launch_bounds__(TILE) void k_ls_init(aoc_params prm, int nspec, int Bp, const real* __restrict__ J_cur,
                                                  const real* __restrict__ descent,
                                                  const real* __restrict__ J_trial, real* __restrict__ stepsize,
                                                  int* __restrict__ ntrials, LsScratch sc, LsFrozen frozen) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane;
    // verdicts of the nspec trials evaluated by aoc_forward, in the reference's order
    const real JP = J_cur[b], d = descent[b];
    real a = prm.stepsize_0;
    bool searching = true;
    int ntr = 0;
    real acc = a;
    for (int j = 0; j < nspec && j < prm.armijo_maxiters; j++) {
        if (searching) {
            ntr = j + 1;
            if (!armijo_reject(J_trial[(size_t)j * Bp + b], JP, prm.cc, a, d)) { searching = false; acc = a; }
        }
        a = prm.beta * a;
    }
    if (frozen.orig) {
        const int ob = frozen.orig[b];
        if (ob < 0 || frozen.ret[ob] != -2) { searching = false; acc = R(0.0); ntr = 0; }
    }
    const unsigned long long m = __ballot(searching);
    stepsize[b] = acc;
    ntrials[b] = ntr;
    sc.first_ok[b] = LS_NOT_FOUND;
    if (lane == 0) sc.mask[tile] = m;
    if (tile == 0 && lane == 0) {
        real al = prm.stepsize_0;
        sc.st->alpha[0] = al;
        for (int i = 1; i <= prm.armijo_maxiters; i++) { al = prm.beta * al; sc.st->alpha[i] = al; }  // optcon.py:270
        const int done = nspec < prm.armijo_maxiters ? nspec : prm.armijo_maxiters;
        sc.st->r_next = done;
        sc.st->r_start = done;
        sc.st->K = 0;
        sc.st->count = 0;
        sc.st->nw = 0;
        sc.st->round = 0;
        sc.st->scheme = 0;
    }
}

// resolve one tile's searching lanes against first_ok; returns the updated mask (lane-parallel)
__device__ __forceinline__ unsigned long long ls_resolve(unsigned long long m, int b, int r_done,
                                                         const LsState* st, int* __restrict__ first_ok,
                                                         real* __restrict__ stepsize, int* __restrict__ ntrials,
                                                         int lane) {
    const bool searching = (m >> lane) & 1ull;
    bool still = false;
    if (searching) {
        const int f = first_ok[b];
        if (f != LS_NOT_FOUND) { stepsize[b] = st->alpha[f]; ntrials[b] = f + 1; }
        else { ntrials[b] = r_done; still = true; }
    }
    return __ballot(still);
}

// work-list search: every candidate of a searching lane has been tried by now; returns the mask of exhausted lanes
__device__ __forceinline__ unsigned long long ls_resolve_wl(unsigned long long m, int b, const LsState* st,
                                                            const int* __restrict__ first_ok, real* __restrict__ stepsize,
                                                            int* __restrict__ ntrials, int lane) {
    bool still = false;
    if ((m >> lane) & 1ull) {
        const int f = first_ok[b];
        if (f != LS_NOT_FOUND) { stepsize[b] = st->alpha[f]; ntrials[b] = f + 1; }
        else still = true;
    }
    return __ballot(still);
}

// resolve the previous round tile by tile (one wavefront per tile)
__global__ __launch_bounds__(TILE) void k_ls_resolve(LsScratch sc, real* __restrict__ stepsize,
                                                     int* __restrict__ ntrials) {
    const int tile = blockIdx.x, lane = threadIdx.x;
    const LsState* st = sc.st;
    if (st->K <= 0) return;
    const unsigned long long m = sc.mask[tile];
    if (m == 0ull) return;
    const unsigned long long m2 = ls_resolve(m, tile * TILE + lane, st->r_next, st, sc.first_ok, stepsize, ntrials, lane);
    if (lane == 0) sc.mask[tile] = m2;
}

// One workgroup: exclusive prefix sum of the per-tile popcounts and the plan of the next round:
// K candidate steps per searching trajectory, as many as keep the round within `wcap` wavefronts,
// but not more than round+1 (rejection thins out geometrically: deep speculation only pays late).
__global__ __launch_bounds__(1024) void k_ls_plan(int ntiles, int maxiters, int wcap, int kgrow, int last_round,
                                                  LsScratch sc) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    LsState* st = sc.st;
    const int r_done = st->r_next;  // indices < r_next have been evaluated for every searching lane
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < ntiles; base += 1024) {
        const int i = base + tid;
        const int c = (i < ntiles) ? __popcll(sc.mask[i]) : 0;
        int incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wv; w++) woff += wsum[w];
        const int carry = carry_s;
        if (i < ntiles) sc.prefix[i] = carry + woff + incl - c;
        __syncthreads();
        if (tid == 1023) carry_s = carry + woff + incl;
        __syncthreads();
    }
    if (tid == 0) {
        const int count = carry_s;
        sc.prefix[ntiles] = count;
        const int nw = (count + TILE - 1) / TILE;
        const int round = st->round + 1;
        int K = 0;
        if (count > 0 && r_done < maxiters) {
            K = wcap / nw;
            if (K > kgrow * round + 1) K = kgrow * round + 1;
            if (K < 1) K = 1;
            if (K > maxiters - r_done || last_round) K = maxiters - r_done;  // the last round takes all that is left
        }
        st->round = round;
        st->r_start = r_done;
        st->K = K;
        st->count = count;
        st->nw = nw;
        st->r_next = r_done + K;
    }
}

__device__ __forceinline__ int nth_set_bit(unsigned long long m, int rank) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const unsigned long long low = m & ((1ull << w) - 1ull);
        const int c = __popcll(low);
        if (rank >= c) { rank -= c; m >>= w; pos += w; }
        else m = low;
    }
    return pos;
}

// item j of the work list -> (tile, home lane): tile with prefix[tile] <= j < prefix[tile+1]
__device__ __forceinline__ void ls_locate(const LsScratch& sc, int ntiles, int j, int& tile, int& hl) {
    const int* __restrict__ prefix = sc.prefix;
    int lo = 0, hi = ntiles;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= j) lo = mid; else hi = mid;
    }
    tile = lo;
    hl = nth_set_bit(sc.mask[lo], j - prefix[lo]);
}

template <bool DIAG, bool RPT>
__global__ __launch_bounds__(TILE) void k_ls_trial(KConst k, aoc_params prm, const real* __restrict__ ref,
                                                   const real* __restrict__ u, const real* __restrict__ x0,
                                                   const real* __restrict__ du, const real* __restrict__ J_cur,
                                                   const real* __restrict__ descent, LsScratch sc) {
    const LsState* st = sc.st;
    const int K = st->K, nw = st->nw;
    const int w = blockIdx.x;
    if (w >= K * nw) return;
    const int kidx = w / nw, slot = w - kidx * nw;
    const int r = st->r_start + kidx;
    const real a_r = st->alpha[r];
    const int count = st->count;
    const int lane = threadIdx.x;
    const int first = slot * TILE;
    const bool valid = first + lane < count;
    int tile, hl;
    ls_locate(sc, k.ntiles, valid ? first + lane : count - 1, tile, hl);  // idle lanes shadow the last item
    const int b = tile * TILE + hl;
    real xs[6];
#pragma unroll
    for (int c = 0; c < 6; c++) xs[c] = x0[((size_t)tile * 6 + c) * TILE + hl];
    int f2 = 0;
    const real Jt = rollout<DIAG, RPT, false, real>(k, ref, tile, hl, xs, u, du, a_r, false, nullptr, nullptr, f2);
    if (valid && !armijo_reject(Jt, J_cur[b], prm.cc, a_r, descent[b])) atomicMin(&sc.first_ok[b], r);
}

// ---------------------------------------------------------------------------------------------
// Work-list line search (large batches).  A work item is (trajectory, CPL consecutive candidate steps), CPL = 1 by
// default: a single rollout chain already keeps its SIMD's fp64 pipe ~75 % busy, so what counts is how many
// independent items are in flight and how few rounds (one rollout latency each, ~0.3 ms at T = 500) there are.
//   k_ls_init_wl  : verdicts of the trials evaluated by aoc_forward; number of trajectories still searching;
//                   per-trajectory PREDICTION of how many further candidates it needs, from its trial count in the
//                   previous iteration (`ntrials` on entry): one more than it needed then, every remaining one if it
//                   exhausted the search (the "exhaustion storms" of long fixed-iteration runs)
//   k_ls_plan_wl  : list of round 0 — every remaining candidate of every searching trajectory if that fits
//                   `cap_items` (about one wavefront per SIMD: the usual case from the third iteration on, ~5 % of
//                   the trajectories searching), the predicted number otherwise
//   k_ls_trial_wl : one wavefront per 64 items; an accepted candidate lowers first_ok[b] (atomicMin)
//   k_ls_replan   : resolve a round; what the prediction missed goes on the next list with every remaining candidate
// The reference tries the same steps one after the other and takes the first that passes: so does the minimum
// over the accepted indices, whatever was predicted — step, trial count and iterate do not depend on the schedule.
// Items of one trajectory are neighbours on the list (their lanes read the same (u, du) addresses: one request),
// items of one tile are contiguous (tiles in arbitrary order: one atomicAdd per tile allocates the slots).
// CPL > 1 (aoc_tuning.ls_cpl = 2, 4) lets a lane carry several chains from one read of (u, du): less traffic, but
// the chains of a lane share one instruction stream — measured slower in every regime (EXPERIMENTS.md).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void ls_put_items(const LsScratch& sc, int round, int lane, int b, int r, int depth, int cpl) {
    const int nit = (depth + cpl - 1) / cpl;
    int incl = nit;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    const int total = __shfl(incl, 63);
    if (total == 0) return;   // wave-uniform
    int base = 0;
    if (lane == 63) base = atomicAdd(&sc.wl_count[round], total);
    base = __shfl(base, 63);
    int pos = base + incl - nit;
    for (int c = 0; c < nit; c++) {
        const int n = depth - c * cpl < cpl ? depth - c * cpl : cpl;
        sc.items[pos + c] = make_int2(b, (r + c * cpl) | (n << 8));
    }
}

__global__ __launch_bounds__(TILE) void k_ls_init_wl(aoc_params prm, int nspec, int cpl, int depth_min, int Bp,
                                                     const real* __restrict__ J_cur, const real* __restrict__ descent,
                                                     const real* __restrict__ J_trial, real* __restrict__ stepsize,
                                                     int* __restrict__ ntrials, LsScratch sc, LsFrozen frozen) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane;
    const int hint = ntrials[b];   // trial count of the previous iteration (anything on the first call): scheduling only
    const real JP = J_cur[b], d = descent[b];
    real a = prm.stepsize_0;
    bool searching = true;
    int ntr = 0;
    real acc = a;
    for (int j = 0; j < nspec && j < prm.armijo_maxiters; j++) {
        if (searching) {
            ntr = j + 1;
            if (!armijo_reject(J_trial[(size_t)j * Bp + b], JP, prm.cc, a, d)) { searching = false; acc = a; }
        }
        a = prm.beta * a;
    }
    if (frozen.orig) {
        const int ob = frozen.orig[b];
        if (ob < 0 || frozen.ret[ob] != -2) { searching = false; acc = R(0.0); ntr = 0; }
    }
    const unsigned long long m = __ballot(searching);
    stepsize[b] = acc;
    ntrials[b] = ntr;
    sc.first_ok[b] = LS_NOT_FOUND;
    if (lane == 0) sc.mask[tile] = m;
    if (tile == 0 && lane == 0) {
        real al = prm.stepsize_0;
        sc.st->alpha[0] = al;
        for (int i = 1; i <= prm.armijo_maxiters; i++) { al = prm.beta * al; sc.st->alpha[i] = al; }  // optcon.py:270
        sc.st->scheme = 1;
    }
    if (m == 0ull) return;
    if (lane == 0) atomicAdd(&sc.wl_count[LS_WL_ROUNDS], __popcll(m));   // trajectories still searching
    const int done = nspec < prm.armijo_maxiters ? nspec : prm.armijo_maxiters;
    const int remaining = prm.armijo_maxiters - done;
    int depth = 0;
    if (searching && remaining > 0) {
        depth = hint >= prm.armijo_maxiters ? remaining : hint - done + 1;
        if (depth < depth_min) depth = depth_min;
        depth = (depth + cpl - 1) / cpl * cpl;   // whole items
        if (depth > remaining) depth = remaining;
    }
    sc.next_r[b] = depth;   // k_ls_plan_wl turns the prediction into the progress marker
}

__global__ __launch_bounds__(TILE) void k_ls_plan_wl(int maxiters, int nspec, int cpl, int cap_items, LsScratch sc) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane;
    const unsigned long long m = sc.mask[tile];
    if (m == 0ull) return;
    const int done = nspec < maxiters ? nspec : maxiters;
    const int remaining = maxiters - done;
    const bool all = (long)sc.wl_count[LS_WL_ROUNDS] * ((remaining + cpl - 1) / cpl) <= (long)cap_items;
    int depth = 0;
    if ((m >> lane) & 1ull) {
        depth = all ? remaining : sc.next_r[b];
        if (depth > LS_WL_IPL * cpl) depth = LS_WL_IPL * cpl;
        sc.next_r[b] = done + depth;
    }
    ls_put_items(sc, 0, lane, b, done, depth, cpl);
}

// resolve the round before `round` and put what is still searching on the list of `round` with every remaining candidate
__global__ __launch_bounds__(TILE) void k_ls_replan(int maxiters, int cpl, int round, real* __restrict__ stepsize,
                                                    int* __restrict__ ntrials, LsScratch sc) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane;
    const unsigned long long m = sc.mask[tile];
    if (m == 0ull) return;
    bool still = false;
    int depth = 0, r = 0;
    if ((m >> lane) & 1ull) {
        const int f = sc.first_ok[b];
        if (f != LS_NOT_FOUND) { stepsize[b] = sc.st->alpha[f]; ntrials[b] = f + 1; }
        else {
            still = true;
            r = sc.next_r[b];
            depth = maxiters - r;
            if (depth > LS_WL_IPL * cpl) depth = LS_WL_IPL * cpl;
            sc.next_r[b] = r + depth;
        }
    }
    const unsigned long long m2 = __ballot(still);
    if (lane == 0) sc.mask[tile] = m2;
    ls_put_items(sc, round, lane, b, r, depth, cpl);
}

// CPL cost-only rollouts of one trajectory with the steps a[0..CPL-1] from one read of (u, du); per chain the
// operations of rollout<DIAG, false, .>, so every cost is bit-identical to a single-candidate trial.
// PF: stages of (u, du) loads in flight (a register ring: 4 doubles per stage).  A lone wavefront needs the deep ring
// (ROLL_PF); in a crowded round the other wavefronts of the SIMD hide the latency and the registers are worth more as
// occupancy (LS_WL_PF).
template <bool DIAG, bool RPT, int CPL, int PF = ROLL_PF>
__device__ __forceinline__ void rollout_multi(const KConst& k, const real* __restrict__ ref, int tile, int lane,
                                              const real* __restrict__ x0, const real* __restrict__ u,
                                              const real* __restrict__ du, const real a[CPL], real Jout[CPL],
                                              const TrigK<real>& tk = TrigK<real>()) {
    constexpr int ROLL_PF = PF;   // (shadows the global depth inside this function)
    const int T = k.T;
    real xs[CPL][6], JJ[CPL], q[6], r[2], rb[8];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const real v = x0[((size_t)tile * 6 + c) * TILE + lane];
#pragma unroll
        for (int j = 0; j < CPL; j++) xs[j][c] = v;
    }
#pragma unroll
    for (int j = 0; j < CPL; j++) JJ[j] = R(0.0);
    real ub[ROLL_PF][2], db[ROLL_PF][2];
#pragma unroll
    for (int i = 0; i < ROLL_PF; i++) {
        const int t = i < T - 1 ? i : T - 2;
        ub[i][0] = u[tix<2>(tile, T, t, 0, lane)];
        ub[i][1] = u[tix<2>(tile, T, t, 1, lane)];
        db[i][0] = du[tix<2>(tile, T, t, 0, lane)];
        db[i][1] = du[tix<2>(tile, T, t, 1, lane)];
    }
    for (int t0 = 0; t0 < T - 1; t0 += ROLL_PF) {
#pragma unroll
        for (int i = 0; i < ROLL_PF; i++) {
            const int t = t0 + i;
            if (t >= T - 1) break;
            const real uc0 = ring_take(ub[i][0]), uc1 = ring_take(ub[i][1]), dc0 = ring_take(db[i][0]), dc1 = ring_take(db[i][1]);
            {
                const int tn = t + ROLL_PF < T - 1 ? t + ROLL_PF : T - 2;
                ub[i][0] = u[tix<2>(tile, T, tn, 0, lane)];
                ub[i][1] = u[tix<2>(tile, T, tn, 1, lane)];
                db[i][0] = du[tix<2>(tile, T, tn, 0, lane)];
                db[i][1] = du[tix<2>(tile, T, tn, 1, lane)];
            }
            const real* rr = ref_row<RPT>(k, ref, tile, lane, t, rb);
#pragma unroll
            for (int j = 0; j < CPL; j++) {
                real u0, u1, xn[6];
                step_inputs(uc0, uc1, a[j], dc0, dc1, u0, u1);
                JJ[j] += stage_cost2<DIAG>(k, xs[j], u0, u1, rr, q, r);
                const SC s = trig(xs[j][3], xs[j][5], tk);
                step_state(k, xs[j], u0, u1, s, xn);
#pragma unroll
                for (int c = 0; c < 6; c++) xs[j][c] = xn[c];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CPL; j++) {
        JJ[j] += term_cost2<DIAG>(k, xs[j], ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
        Jout[j] = R(0.5) * JJ[j];  // JJ accumulated twice the cost, see stage_cost2
    }
}

template <bool DIAG, bool RPT, int CPL, int PF = ROLL_PF>
__device__ __forceinline__ void ls_trial_item(const KConst& k, const aoc_params& prm, const real* __restrict__ ref,
                                              const real* __restrict__ u, const real* __restrict__ x0,
                                              const real* __restrict__ du, const real* __restrict__ J_cur,
                                              const real* __restrict__ descent, const LsScratch& sc, int b, int r0, int n,
                                              const TrigK<real>& tk = TrigK<real>()) {
    real a[CPL], J[CPL];
#pragma unroll
    for (int j = 0; j < CPL; j++) a[j] = sc.st->alpha[r0 + (j < n ? j : 0)];   // spare chains repeat the first step
    rollout_multi<DIAG, RPT, CPL, PF>(k, ref, b / TILE, b % TILE, x0, u, du, a, J, tk);
    if (n <= 0) return;
    const real JP = J_cur[b], d = descent[b];
    int acc = -1;
#pragma unroll
    for (int j = CPL - 1; j >= 0; j--)
        if (j < n && !armijo_reject(J[j], JP, prm.cc, a[j], d)) acc = j;
    if (acc >= 0) atomicMin(&sc.first_ok[b], r0 + acc);
}

// PIN: a round of at most LS_WL_PIN_ITEMS items has a SIMD per wavefront (the search of an ordinary iteration: 5 % of the
// trajectories, ~800 wavefronts), and a lone wavefront pays for every scalar instruction and scalar load of the
// rollout (EXPERIMENTS.md): that build keeps its constants in VGPRs (pin_consts).  The other build serves the crowded
// rounds, where registers are occupancy.  Both are launched; the one whose regime it is not exits at once.
#ifndef AOC_LS_WL_PIN_ITEMS
#define AOC_LS_WL_PIN_ITEMS (1024 * TILE)
#endif
constexpr int LS_WL_PIN_ITEMS = AOC_LS_WL_PIN_ITEMS;
#ifndef AOC_LS_WL_PF
#define AOC_LS_WL_PF 8
#endif
constexpr int LS_WL_PF = AOC_LS_WL_PF;   // ring depth of the crowded rounds' build
template <bool DIAG, bool RPT, int CPL, bool PIN>
__global__ __launch_bounds__(TILE) void k_ls_trial_wl(KConst kc, aoc_params prm, int round, const real* __restrict__ ref,
                                                      const real* __restrict__ u, const real* __restrict__ x0,
                                                      const real* __restrict__ du, const real* __restrict__ J_cur,
                                                      const real* __restrict__ descent, LsScratch sc) {
    const int count = sc.wl_count[round];
    const int first = blockIdx.x * TILE, lane = threadIdx.x;
    if (first >= count || (CPL == 1 && PIN != (count <= LS_WL_PIN_ITEMS))) return;
    KConst k = kc;
    TrigK<real> tk;
    if (PIN) { pin_consts<DIAG>(k); pin_trig(tk); }
    const bool valid = first + lane < count;
    const int2 it = sc.items[valid ? first + lane : count - 1];   // idle lanes shadow the last item
    ls_trial_item<DIAG, RPT, CPL, (PIN ? ROLL_PF : LS_WL_PF)>(k, prm, ref, u, x0, du, J_cur, descent, sc, it.x, it.y & 0xff,
                                                               valid ? it.y >> 8 : 0, tk);
}

template <bool DIAG, bool RPT, typename XO>
__global__ __launch_bounds__(TILE) void k_ls_final(KConst k, int maxiters, const real* __restrict__ ref,
                                                   const real* __restrict__ u, const real* __restrict__ x0,
                                                   const real* __restrict__ du, XO* __restrict__ x_new,
                                                   real* __restrict__ u_new, real* __restrict__ J_new,
                                                   real* __restrict__ stepsize, int* __restrict__ ntrials,
                                                   int* __restrict__ status, LsScratch sc) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane;
    const LsState* st = sc.st;
    int flags = 0;
    const unsigned long long m = sc.mask[tile];
    if (m != 0ull) {  // resolve the last round (by the scheme the search recorded); what is still searching has exhausted the line search
        const unsigned long long left = st->scheme ? ls_resolve_wl(m, b, st, sc.first_ok, stepsize, ntrials, lane)
                                         : (st->K > 0) ? ls_resolve(m, b, st->r_next, st, sc.first_ok, stepsize, ntrials, lane) : m;
        if ((left >> lane) & 1ull) {
            stepsize[b] = st->alpha[maxiters];  // never evaluated (Q5, optcon.py:327)
            ntrials[b] = maxiters;
            flags |= AOC_ST_ARMIJO_EXH;
        }
    }
    const real a = stepsize[b];
    real xs[6];
#pragma unroll
    for (int c = 0; c < 6; c++) xs[c] = x0[((size_t)tile * 6 + c) * TILE + lane];
    const real Jf = rollout<DIAG, RPT, true, XO>(k, ref, tile, lane, xs, u, du, a, true, x_new, u_new, flags);
    if (Jf != Jf || Jf - Jf != R(0.0)) flags |= AOC_ST_NAN;
    J_new[b] = Jf;
    if (status && flags) status[b] |= flags;
}

// Small batches: a state-writing rollout on two wavefronts per tile.  Wavefront 0 (`chain`) carries the state
// chain (u' = u + a du, sin/cos, step, x' stores) and publishes (x_t, u'_t) through LDS; wavefront 1, one stage
// behind, accumulates the cost of the new iterate and stores u'.  Same operations as rollout<DIAG, true, XO>,
// results bit-identical.  Returns the cost in wavefront 1 (0 in wavefront 0); T barriers on both paths.
// WRITE = false: cost only (Armijo trials; x_new, u_new unused).  `lane` indexes the trajectory inside its tile
// in global memory, `ll` is the thread's own lane (its LDS column): they differ for compacted work lists.
// SHIFT = 1: the inputs are read one sample ahead, u_t := u[min(t + 1, T - 2)] (the receding-horizon shift: the last input
// repeats) — k_mpc_warm_split rolls out the shifted inputs without writing them anywhere first.
template <bool DIAG, bool RPT, typename XO, bool WRITE = true, int SHIFT = 0>
__device__ __forceinline__ real rollout_split(const KConst& k, const real* __restrict__ ref, int tile, int lane, bool chain,
                                              real a, const real* __restrict__ x0, const real* __restrict__ u,
                                              const real* __restrict__ du, XO* __restrict__ x_new,
                                              real* __restrict__ u_new, real (*sh)[4][TILE][2], int& flags, int ll = -1,
                                              const TrigK<real>& tk = TrigK<real>(), const real* xs0 = nullptr) {
    // xs0 (chain wavefront only): the initial state in registers instead of x0[] — for a caller that has just computed it
    // (k_mpc_warm_split) and would otherwise read its own global store back
    const int T = k.T;
    if (ll < 0) ll = lane;
    if (chain) {
        real xs[6], xn[6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            xs[c] = xs0 ? xs0[c] : x0[((size_t)tile * 6 + c) * TILE + lane];
            if (WRITE) x_new[tix<6>(tile, T, 0, c, lane)] = (XO)xs[c];
        }
        // The ring turns in every stage and is fed unconditionally — from u itself when there is no direction, the
        // values then replaced by zero where they are used: every path through the loop body issues the same loads, so
        // the compiler keeps count of what is in flight (see k_forward_split)
        const bool has_du = du != nullptr;
        const real* __restrict__ dsrc = has_du ? du : u;
        real ub[ROLL_PF][2], db[ROLL_PF][2];
#pragma unroll
        for (int i = 0; i < ROLL_PF; i++) {
            const int t = i + SHIFT < T - 1 ? i + SHIFT : T - 2;
            ub[i][0] = u[tix<2>(tile, T, t, 0, lane)];
            ub[i][1] = u[tix<2>(tile, T, t, 1, lane)];
            db[i][0] = dsrc[tix<2>(tile, T, t, 0, lane)];
            db[i][1] = dsrc[tix<2>(tile, T, t, 1, lane)];
        }
        for (int t0 = 0; t0 < T; t0 += ROLL_PF) {
#pragma unroll
            for (int i = 0; i < ROLL_PF; i++) {
                const int t = t0 + i;
                if (t >= T) break;
                real(*dst)[TILE][2] = sh[t & 1];
#pragma unroll
                for (int c = 0; c < 6; c++) dst[c >> 1][ll][c & 1] = xs[c];
                const real uc0 = ring_take(ub[i][0]), uc1 = ring_take(ub[i][1]), dt0 = ring_take(db[i][0]), dt1 = ring_take(db[i][1]);
                const real dc0 = has_du ? dt0 : R(0.0), dc1 = has_du ? dt1 : R(0.0);
                {
                    const int tn = t + ROLL_PF + SHIFT < T - 1 ? t + ROLL_PF + SHIFT : T - 2;
                    ub[i][0] = u[tix<2>(tile, T, tn, 0, lane)];
                    ub[i][1] = u[tix<2>(tile, T, tn, 1, lane)];
                    db[i][0] = dsrc[tix<2>(tile, T, tn, 0, lane)];
                    db[i][1] = dsrc[tix<2>(tile, T, tn, 1, lane)];
                }
                if (t < T - 1) {
                    real u0, u1;
                    step_inputs(uc0, uc1, a, dc0, dc1, u0, u1);
                    dst[3][ll][0] = u0; dst[3][ll][1] = u1;
                    const SC s = trig(xs[3], xs[5], tk);
                    step_state(k, xs, u0, u1, s, xn);
#pragma unroll
                    for (int c = 0; c < 6; c++) { if (WRITE) x_new[tix<6>(tile, T, t + 1, c, lane)] = (XO)xn[c]; xs[c] = xn[c]; }
                }
                __syncthreads();
            }
        }
        return R(0.0);
    }
    real xs[6], q[6], r[2], rb[8], JJ = R(0.0);
    for (int step = 0; step < T; step++) {
        if (step >= 1) {
            const int t = step - 1;
            real(*src)[TILE][2] = sh[t & 1];
#pragma unroll
            for (int c = 0; c < 6; c++) xs[c] = src[c >> 1][ll][c & 1];
            const real u0 = src[3][ll][0], u1 = src[3][ll][1];
            JJ += stage_cost2<DIAG>(k, xs, u0, u1, ref_row<RPT>(k, ref, tile, lane, t, rb), q, r);
            if (WRITE) {   // trials are silent: only the update reports
                if (!(xs[2] > R(0.0))) flags |= AOC_ST_VNONPOS;
                u_new[tix<2>(tile, T, t, 0, lane)] = u0;
                u_new[tix<2>(tile, T, t, 1, lane)] = u1;
            }
        }
        __syncthreads();
    }
    {
        real(*src)[TILE][2] = sh[(T - 1) & 1];
#pragma unroll
        for (int c = 0; c < 6; c++) xs[c] = src[c >> 1][ll][c & 1];
    }
    JJ += term_cost2<DIAG>(k, xs, ref_row<RPT>(k, ref, tile, lane, T - 1, rb), q);
    if (WRITE) {
        u_new[tix<2>(tile, T, T - 1, 0, lane)] = R(0.0);  // optcon.py:193: uu_temp[:, T-1] stays 0
        u_new[tix<2>(tile, T, T - 1, 1, lane)] = R(0.0);
    }
    return R(0.5) * JJ;  // JJ accumulated twice the cost, see stage_cost2
}

// grid (tiles, LSF_NY).  A tile whose trajectories all accepted a candidate the forward pass stored (CandBuf) is
// updated by copying: block y takes the samples t = y, y + LSF_NY, ...; any other tile is rolled out by its block 0.
#ifndef AOC_LSF_NY
#define AOC_LSF_NY 32
#endif
constexpr int LSF_NY = AOC_LSF_NY;
template <bool DIAG, bool RPT, typename XO>
__global__ __launch_bounds__(2 * TILE) void k_ls_final_split(KConst kc, int maxiters, CandBuf cb,
                                                             const real* __restrict__ J_trial, const real* __restrict__ ref,
                                                             const real* __restrict__ u, const real* __restrict__ x0,
                                                             const real* __restrict__ du, XO* __restrict__ x_new,
                                                             real* __restrict__ u_new, real* __restrict__ J_new,
                                                             real* __restrict__ stepsize, int* __restrict__ ntrials,
                                                             int* __restrict__ status, LsScratch sc) {
    __shared__ __attribute__((aligned(16))) real sh[2][4][TILE][2];   // state and input pairs per lane, 16-byte accesses
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), b = tile * TILE + lane, T = kc.T;
    const bool chain = threadIdx.x < TILE;
    if (cb.n > 0) {
        // read-only test, the same in every block of the tile.  A store exists only where every candidate rode along in
        // the forward pass (n_spec >= armijo_maxiters), so k_ls_init has judged them all and a set mask bit means an
        // EXHAUSTED search: it applies candidate index maxiters, the never-judged step (Q5), which is stored when
        // n_spec > maxiters.  ntrials = 0 marks a lane frozen by aoc_newton_solve (stopped trajectory: whatever is
        // written for it is never read again): it takes candidate 0.  The tile is copied if every lane's step is stored.
        const int ntr = ntrials[b], nst = cb.nstored[tile];
        const bool exh = (sc.mask[tile] >> lane) & 1ull;
        const bool lane_ok = exh ? (cb.n > maxiters && nst > maxiters) : ntr <= nst;
        const bool stored = __ballot(!lane_ok) == 0ull;   // block-uniform
        if (stored) {
            const int a = exh ? maxiters : (ntr >= 1 ? ntr - 1 : 0), Bp = kc.ntiles * TILE;
            const cand2* __restrict__ crec = cb.rec + cand_ix(a, kc.ntiles, tile, T, 0, 0, lane);
            const real al = sc.st->alpha[a];     // alpha_a as the trial wavefront formed it (k_ls_init: the same recurrence)
            // record t holds x'_{t+1}; u'_t = u_t + alpha_a du_t re-computed (optcon.py:253); x'_0 = x0, u'_{T-1} = 0 (optcon.py:193)
            for (int t = blockIdx.y * 2 + (chain ? 0 : 1); t < T; t += 2 * gridDim.y) {
                if (t < T - 1) {
                    const real uc0 = u[tix<2>(tile, T, t, 0, lane)], uc1 = u[tix<2>(tile, T, t, 1, lane)];
                    const real d0 = du[tix<2>(tile, T, t, 0, lane)], d1 = du[tix<2>(tile, T, t, 1, lane)];
                    cand2 v[3];
#pragma unroll
                    for (int h = 0; h < 3; h++) v[h] = crec[((size_t)t * 3 + h) * TILE];
                    real u0, u1;
                    step_inputs(uc0, uc1, al, d0, d1, u0, u1);
                    u_new[tix<2>(tile, T, t, 0, lane)] = u0;
                    u_new[tix<2>(tile, T, t, 1, lane)] = u1;
#pragma unroll
                    for (int h = 0; h < 3; h++) {
                        x_new[tix<6>(tile, T, t + 1, 2 * h, lane)] = (XO)v[h].x;
                        x_new[tix<6>(tile, T, t + 1, 2 * h + 1, lane)] = (XO)v[h].y;
                    }
                } else {
                    u_new[tix<2>(tile, T, t, 0, lane)] = R(0.0);
                    u_new[tix<2>(tile, T, t, 1, lane)] = R(0.0);
                }
                if (t == 0) {
#pragma unroll
                    for (int c = 0; c < 6; c++) x_new[tix<6>(tile, T, 0, c, lane)] = (XO)x0[((size_t)tile * 6 + c) * TILE + lane];
                }
            }
            if (blockIdx.y == 0 && chain) {
                const real Jf = J_trial[(size_t)a * Bp + b];
                int flags = cb.flags[(size_t)a * Bp + b];
                if (Jf != Jf || Jf - Jf != R(0.0)) flags |= AOC_ST_NAN;
                if (exh) {   // what the rollout path records for an exhausted search (ntrials already holds maxiters)
                    stepsize[b] = sc.st->alpha[maxiters];
                    flags |= AOC_ST_ARMIJO_EXH;
                }
                J_new[b] = Jf;
                if (status && flags && (ntr >= 1 || exh)) atomicOr(&status[b], flags);
            }
            return;
        }
    }
    if (blockIdx.y != 0) return;
    AOC_PINNED_CONSTS(DIAG)
    int flags = 0;
    real a = R(0.0);
    if (chain) {
        const LsState* st = sc.st;
        const unsigned long long m = sc.mask[tile];
        if (m != 0ull) {  // resolve the last round (by the scheme the search recorded); what is still searching has exhausted the line search
            const unsigned long long left = st->scheme ? ls_resolve_wl(m, b, st, sc.first_ok, stepsize, ntrials, lane)
                                             : (st->K > 0) ? ls_resolve(m, b, st->r_next, st, sc.first_ok, stepsize, ntrials, lane) : m;
            if ((left >> lane) & 1ull) {
                stepsize[b] = st->alpha[maxiters];  // never evaluated (Q5, optcon.py:327)
                ntrials[b] = maxiters;
                flags |= AOC_ST_ARMIJO_EXH;
            }
        }
        a = stepsize[b];
    }
    const real Jf = rollout_split<DIAG, RPT, XO>(k, ref, tile, lane, chain, a, x0, u, du, x_new, u_new, sh, flags, -1, tk);
    if (!chain) {
        if (Jf != Jf || Jf - Jf != R(0.0)) flags |= AOC_ST_NAN;
        J_new[b] = Jf;
    }
    if (status && flags) atomicOr(&status[b], flags);
}

// get_update / trial cost with stored states for small batches (see rollout_split)
template <bool DIAG, bool RPT, typename XO>
__global__ __launch_bounds__(2 * TILE) void k_rollout_cost_split(KConst kc, const real* __restrict__ ref,
                                                                 const real* __restrict__ x0, const real* __restrict__ u,
                                                                 const real* __restrict__ du, const real* __restrict__ alpha,
                                                                 XO* __restrict__ x_out, real* __restrict__ u_out,
                                                                 real* __restrict__ J_out, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) real sh[2][4][TILE][2];   // state and input pairs per lane, 16-byte accesses
    AOC_PINNED_CONSTS(DIAG)
    const int tile = blockIdx.x, lane = threadIdx.x & (TILE - 1), b = tile * TILE + lane;
    const bool chain = threadIdx.x < TILE;
    int flags = 0;
    const real a = (du && alpha) ? alpha[b] : R(0.0);
    const real Jf = rollout_split<DIAG, RPT, XO>(k, ref, tile, lane, chain, a, x0, u, du, x_out, u_out, sh, flags, -1, tk);
    if (!chain) {
        if (Jf != Jf || Jf - Jf != R(0.0)) flags |= AOC_ST_NAN;
        J_out[b] = Jf;
    }
    if (status && flags) atomicOr(&status[b], flags);
}

// Trial rounds on two wavefronts per work item (state chain / cost), for the rounds that are bound by the latency
// of one rollout rather than by bandwidth: the gathered rounds of batches of at most 512 tiles.
template <bool DIAG, bool RPT>
__global__ __launch_bounds__(2 * TILE) void k_ls_trial_split(KConst kc, aoc_params prm, const real* __restrict__ ref,
                                                             const real* __restrict__ u, const real* __restrict__ x0,
                                                             const real* __restrict__ du, const real* __restrict__ J_cur,
                                                             const real* __restrict__ descent, LsScratch sc) {
    __shared__ __attribute__((aligned(16))) real sh[2][4][TILE][2];   // state and input pairs per lane, 16-byte accesses
    const LsState* st = sc.st;
    const int K = st->K, nw = st->nw;
    const int w = blockIdx.x;
    if (w >= K * nw) return;   // block-uniform
    AOC_PINNED_CONSTS(DIAG)
    const int kidx = w / nw, slot = w - kidx * nw;
    const int r = st->r_start + kidx;
    const real a_r = st->alpha[r];
    const int count = st->count;
    const int lane = threadIdx.x & (TILE - 1);
    const bool chain = threadIdx.x < TILE;
    const int first = slot * TILE;
    const bool valid = first + lane < count;
    int tile, hl;
    ls_locate(sc, k.ntiles, valid ? first + lane : count - 1, tile, hl);  // idle lanes shadow the last item
    const int b = tile * TILE + hl;
    int f2 = 0;
    const real Jt = rollout_split<DIAG, RPT, real, false>(k, ref, tile, hl, chain, a_r, x0, u, du, (real*)nullptr, nullptr, sh, f2, lane, tk);
    if (!chain && valid && !armijo_reject(Jt, J_cur[b], prm.cc, a_r, descent[b])) atomicMin(&sc.first_ok[b], r);
}

