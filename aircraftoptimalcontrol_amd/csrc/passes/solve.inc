// passes/solve.inc — solve level: NewtonMethod.optimize with per-trajectory termination, re-packing, two streams.
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// Solve level: NewtonMethod.optimize's loop with its per-trajectory termination on the device
// (optcon.py:415-505).  Iterate i >= 1 lives in slot (i-1) % 3 of three rotating buffers, iterate 0 is the
// caller's initial iterate; a trajectory that stops at iteration kk (descent[kk] >= term_cond, Q6) returns
// iterate kk-1 (Q7): k_solve_book copies it out of the buffer two behind the newest while it still exists.
// Trajectories that have stopped are frozen (no line search, step 0).  The host reads the count of iterating
// trajectories at its sync points (every `sync_every` iterations while nobody has stopped, every
// aoc_tuning.solve_sync_fast afterwards) and, when at most aoc_tuning.solve_repack_pct per cent of the batch in flight
// still iterates, the iterating ones are re-packed into a dense smaller batch ("generation"): orig[] maps a lane of
// the generation to the caller's trajectory index, which is where every per-trajectory output goes.  A fourth
// iterate buffer (the spare) lets a re-pack happen at any fraction: the survivors' newest iterate goes into the free
// slot, their previous one into the spare, and the old "previous" slot becomes the next spare.
//
// The all-NaN fixed point.  The reference's stopping test `descent >= -1e-6` is False for a NaN descent (optcon.py:499),
// so a trajectory that has diverged iterates to max_iters — and from the moment every input sample of its iterate is NaN
// nothing changes any more: the states are f(x0, NaN...) (the same partly finite first sample every time), the gains,
// the direction and the new inputs NaN, the first Armijo candidate is "accepted" (NaN > x is False).  k_solve_book
// recognises that iterate (scan of the newest inputs, only in lanes whose descent is NaN); after ONE more iteration has
// run on it (so that every status flag such an iteration raises is raised) the trajectory is retired with exactly what
// the remaining iterations would produce: returned iterate = this one, index max_iters-1, iters = max_iters-1, history
// rows (NaN, NaN, this iteration's step and trial count).  Six such trajectories in 65 536 used to keep ten tiles
// iterating for 22 iterations after everybody else had stopped (21 of 113 ms).
// ---------------------------------------------------------------------------------------------
constexpr int SOLVE_ACTIVE = -2;
constexpr int SOLVE_REPACK_MIN = 2048;  // do not re-pack batches that are already latency-bound
constexpr int SOLVE_ST_PRE = 1 << 30;   // run_status, internal: the newest iterate has been seen to be the all-NaN fixed point

__global__ __launch_bounds__(TILE) void k_solve_init(int B, int* __restrict__ ret, int* __restrict__ iters,
                                                     int* __restrict__ status_out, int* __restrict__ run_status,
                                                     int* __restrict__ orig, int* __restrict__ n_active) {
    const int b = blockIdx.x * TILE + threadIdx.x;
    ret[b] = b < B ? SOLVE_ACTIVE : -1;
    iters[b] = 0;
    status_out[b] = 0;
    run_status[b] = 0;
    orig[b] = b < B ? b : -1;  // padding lanes replicate trajectory B-1 and report nothing
    if (b == 0) { n_active[0] = B; n_active[1] = 0; }
}

// One trajectory (tile, lane of the generation) copied to where the caller's arrays keep it (ot, ol), with
// u_star[:, T-1] = u_star[:, T-2] (optcon.py:505): the samples t = y, y + ny, ... (k_solve_copy: grid (tiles, ny)).
// WITH_X = false: the inputs only.  Every iterate >= 1 is the rollout of its inputs from x0 as this library computes it
// (the line search's update wrote it: same step_state, same roundings), so its states need not travel lane-sparse through
// the caller's rows in every iteration in which trajectories stop — k_solve_restate re-states them once, at the end.
template <typename XS, typename XO, bool WITH_X>
__device__ __forceinline__ void solve_copy_out(int T, int tile, int lane, int ot, int ol, const XS* __restrict__ x_src,
                                               const real* __restrict__ u_src, XO* __restrict__ x_star,
                                               real* __restrict__ u_star, int y, int ny) {
    for (int t = y; t < T; t += ny) {
        const int tu = t == T - 1 ? T - 2 : t;
        const real u0 = u_src[tix<2>(tile, T, tu, 0, lane)], u1 = u_src[tix<2>(tile, T, tu, 1, lane)];
        if (WITH_X) {
            XS xv[6];
#pragma unroll
            for (int c = 0; c < 6; c++) xv[c] = x_src[tix<6>(tile, T, t, c, lane)];
#pragma unroll
            for (int c = 0; c < 6; c++) x_star[tix<6>(ot, T, t, c, ol)] = (XO)xv[c];
        }
        u_star[tix<2>(ot, T, t, 0, ol)] = u0;
        u_star[tix<2>(ot, T, t, 1, ol)] = u1;
    }
}

// final_pass = 0: bookkeeping after iteration kk.  (x_src,u_src) = iterate kk-1 (null for kk = 0: the
//   reference returns its all-zero last history slot then); (x_new,u_new) = iterate kk+1, the newest.
// final_pass = 1: after the last iteration `kk`: what still iterates returns the newest iterate (x_src,u_src),
//   index kk+1.
// n_it = max_iters-1: the iterations the reference runs for a trajectory that never stops.  hstride = row length of
// the history arrays (padded size of the caller's whole batch).
// What k_solve_copy does for a lane: nothing, the returned iterate from (x_src, u_src), from the newest iterate (a retired
// all-NaN trajectory), or the reference's all-zero history slot (a stop at kk = 0).
constexpr int SOLVE_COPY_NONE = 0, SOLVE_COPY_SRC = 1, SOLVE_COPY_NEW = 2, SOLVE_COPY_ZERO = 3;
constexpr int SOLVE_COPY_NY = 16;   // blocks over the horizon per tile in k_solve_copy

// The decisions of an iteration, one lane per trajectory; the trajectories it selects are copied out by k_solve_copy
// (parallel over the horizon: as one serial loop per lane inside this kernel the copy took 0.16-0.18 ms of every tail
// iteration of a converge-mode solve).
__global__ __launch_bounds__(TILE) void k_solve_book(int T, int kk, real term_cond, int final_pass, int n_it,
                                                     const int* __restrict__ orig,
                                                     const real* __restrict__ descent, const real* __restrict__ J_it,
                                                     const real* __restrict__ stepsize, const int* __restrict__ ntrials,
                                                     int* __restrict__ run_status, int* __restrict__ ret,
                                                     int* __restrict__ iters, int* __restrict__ status_out,
                                                     int* __restrict__ n_active, int have_src,
                                                     const real* __restrict__ u_new, int* __restrict__ code,
                                                     real* __restrict__ h_cost,
                                                     real* __restrict__ h_desc, real* __restrict__ h_step,
                                                     int* __restrict__ h_ntr, int hstride) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane;
    const int ob = orig[b];
    const bool active = ob >= 0 && ret[ob] == SOLVE_ACTIVE;
    bool sel, absorb = false;
    if (final_pass) {
        sel = active;
        if (sel) { ret[ob] = kk + 1; status_out[ob] = run_status[b] & ~SOLVE_ST_PRE; }
    } else {
        const real d = descent[b];
        if (active) {
            const size_t h = (size_t)kk * hstride + ob;
            if (h_cost) h_cost[h] = J_it[b];
            if (h_desc) h_desc[h] = d;
            if (h_step) h_step[h] = stepsize[b];
            if (h_ntr) h_ntr[h] = ntrials[b];
            iters[ob] = kk + 1;
        }
        sel = active && d >= term_cond;  // a NaN descent never stops, as in the reference
        if (sel) { ret[ob] = kk - 1; status_out[ob] = (run_status[b] & ~SOLVE_ST_PRE) | AOC_ST_CONVERGED; }
        if (active && d != d && kk + 1 < n_it) {   // the all-NaN fixed point (see above)
            bool all = true;   // (no early exit: the loads then go out back to back instead of one round trip per sample)
#pragma unroll 8
            for (int t = 0; t < T - 1; t++) {
                const real a0 = u_new[tix<2>(tile, T, t, 0, lane)], a1 = u_new[tix<2>(tile, T, t, 1, lane)];
                all = all && a0 != a0 && a1 != a1;
            }
            if (all) {
                const int rs = run_status[b];
                if (rs & SOLVE_ST_PRE) absorb = true;          // this iteration already ran on the fixed point
                else run_status[b] = rs | SOLVE_ST_PRE;
            }
        }
        if (absorb) {
            ret[ob] = n_it;
            iters[ob] = n_it;
            status_out[ob] = run_status[b] & ~SOLVE_ST_PRE;
            const real nan = __builtin_nan("");
            for (int k2 = kk + 1; k2 < n_it; k2++) {
                const size_t h = (size_t)k2 * hstride + ob;
                if (h_cost) h_cost[h] = nan;
                if (h_desc) h_desc[h] = nan;
                if (h_step) h_step[h] = stepsize[b];
                if (h_ntr) h_ntr[h] = ntrials[b];
            }
        }
    }
    code[b] = absorb ? SOLVE_COPY_NEW : sel ? (have_src ? SOLVE_COPY_SRC : SOLVE_COPY_ZERO) : SOLVE_COPY_NONE;
    const unsigned long long m = __ballot(sel || absorb);
    if (m == 0ull) return;
    const unsigned long long ma = __ballot(absorb);
    if (!final_pass && lane == 0) {
        atomicSub(n_active, __popcll(m));
        if (ma) atomicAdd(n_active + 1, __popcll(ma));
    }
}

// grid (tiles of the generation, SOLVE_COPY_NY): the trajectories k_solve_book selected, copied to the caller's arrays.
// src_is_init: (x_src, u_src) is the caller's initial iterate (index 0: arbitrary states, copied as they are); every other
// returned iterate travels as inputs only (see solve_copy_out).
template <typename XS, typename XO>
__global__ __launch_bounds__(TILE) void k_solve_copy(int T, int src_is_init, const int* __restrict__ orig,
                                                     const int* __restrict__ code,
                                                     const XS* __restrict__ x_src, const real* __restrict__ u_src,
                                                     const real* __restrict__ u_new,
                                                     XO* __restrict__ x_star, real* __restrict__ u_star) {
    const int tile = blockIdx.x, lane = threadIdx.x, b = tile * TILE + lane;
    const int c = code[b];
    if (__ballot(c != SOLVE_COPY_NONE) == 0ull) return;
    if (c == SOLVE_COPY_NONE) return;
    const int ob = orig[b], ot = ob / TILE, ol = ob % TILE;  // where the caller's arrays keep this trajectory
    if (c == SOLVE_COPY_NEW)
        solve_copy_out<XS, XO, false>(T, tile, lane, ot, ol, x_src, u_new, x_star, u_star, blockIdx.y, gridDim.y);
    else if (c == SOLVE_COPY_SRC) {
        if (src_is_init) solve_copy_out<XS, XO, true>(T, tile, lane, ot, ol, x_src, u_src, x_star, u_star, blockIdx.y, gridDim.y);
        else solve_copy_out<XS, XO, false>(T, tile, lane, ot, ol, x_src, u_src, x_star, u_star, blockIdx.y, gridDim.y);
    } else {
        for (int t = blockIdx.y; t < T; t += gridDim.y) {
#pragma unroll
            for (int cc = 0; cc < 6; cc++) x_star[tix<6>(ot, T, t, cc, ol)] = (XO)0;
            u_star[tix<2>(ot, T, t, 0, ol)] = R(0.0);
            u_star[tix<2>(ot, T, t, 1, ol)] = R(0.0);
        }
    }
}

// The states of every returned iterate of index >= 1, re-stated from its inputs: x_star = rollout of u_star from x0
// (get_update, optcon.py:176-200; float32 rounding of every state), one wavefront per tile of the caller's batch, lanes
// whose trajectory returned index 0 (the caller's own states) or -1 (zeros) masked.  u_star[:, T-1] (already set to
// u_star[:, T-2], Q8) does not enter a rollout.
template <typename XO>
__global__ __launch_bounds__(TILE) void k_solve_restate(KConst k, const int* __restrict__ ret, const real* __restrict__ x0,
                                                        const real* __restrict__ u_star, XO* __restrict__ x_star) {
    const int tile = blockIdx.x, lane = threadIdx.x, T = k.T;
    const bool on = ret[tile * TILE + lane] >= 1;
    if (__ballot(on) == 0ull) return;
    real xs[6], xn[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        xs[c] = x0[((size_t)tile * 6 + c) * TILE + lane];
        if (on) x_star[tix<6>(tile, T, 0, c, lane)] = (XO)xs[c];
    }
    real ub[ROLL_PF][2];
#pragma unroll
    for (int i = 0; i < ROLL_PF; i++) {
        const int t = i < T - 1 ? i : T - 2;
        ub[i][0] = u_star[tix<2>(tile, T, t, 0, lane)];
        ub[i][1] = u_star[tix<2>(tile, T, t, 1, lane)];
    }
    for (int t0 = 0; t0 < T - 1; t0 += ROLL_PF) {
#pragma unroll
        for (int i = 0; i < ROLL_PF; i++) {
            const int t = t0 + i;
            if (t >= T - 1) break;
            const real u0 = ring_take(ub[i][0]), u1 = ring_take(ub[i][1]);
            {
                const int tn = t + ROLL_PF < T - 1 ? t + ROLL_PF : T - 2;
                ub[i][0] = u_star[tix<2>(tile, T, tn, 0, lane)];
                ub[i][1] = u_star[tix<2>(tile, T, tn, 1, lane)];
            }
            const SC s = trig(xs[3], xs[5]);
            step_state(k, xs, u0, u1, s, xn);
#pragma unroll
            for (int c = 0; c < 6; c++) { if (on) x_star[tix<6>(tile, T, t + 1, c, lane)] = (XO)xn[c]; xs[c] = xn[c]; }
        }
    }
}

// The history rows of an iteration are NaN / -1 for every trajectory that no longer iterates.
__global__ void k_solve_hist_fill(size_t n, real* __restrict__ h_cost, real* __restrict__ h_desc,
                                  real* __restrict__ h_step, int* __restrict__ h_ntr) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const real nan = __builtin_nan("");
    if (h_cost) h_cost[i] = nan;
    if (h_desc) h_desc[i] = nan;
    if (h_step) h_step[i] = nan;
    if (h_ntr) h_ntr[i] = -1;
}

// ---- re-packing: mask of still-iterating lanes per tile, exclusive prefix of the popcounts, gather
__global__ __launch_bounds__(TILE) void k_repack_mask(const int* __restrict__ orig, const int* __restrict__ ret,
                                                      unsigned long long* __restrict__ mask) {
    const int b = blockIdx.x * TILE + threadIdx.x;
    const int ob = orig[b];
    const unsigned long long m = __ballot(ob >= 0 && ret[ob] == SOLVE_ACTIVE);
    if (threadIdx.x == 0) mask[blockIdx.x] = m;
}

__global__ __launch_bounds__(1024) void k_prefix_popc(int ntiles, const unsigned long long* __restrict__ mask,
                                                      int* __restrict__ prefix) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < ntiles; base += 1024) {
        const int i = base + tid;
        const int c = (i < ntiles) ? __popcll(mask[i]) : 0;
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
        if (i < ntiles) prefix[i] = carry + woff + incl - c;
        __syncthreads();
        if (tid == 1023) carry_s = carry + woff + incl;
        __syncthreads();
    }
    if (tid == 0) prefix[ntiles] = carry_s;
}

struct SolveGen {          // one generation's view of the rotating iterate buffers and per-trajectory arrays
    float* x[3];
    real* u[3];
    float* xs;             // the spare iterate buffer (see above)
    real* us;
    const real* x0;
    real* J[2];
    int* run_status;
    int* orig;
    int B;
};

constexpr int LS_GCH = 32;   // stages per workgroup of the re-packing gather
// grid (new tiles, chunks of LS_GCH stages).  Lane j of the new generation takes over the trajectory that is
// the j-th still-iterating one of the old generation (lanes beyond `count` shadow the last one and get orig -1).
__global__ __launch_bounds__(TILE) void k_repack_gather(int T, int ntiles_old, int count, LsScratch sc,
                                                        const float* __restrict__ xa, const float* __restrict__ xb,
                                                        const real* __restrict__ ua, const real* __restrict__ ub,
                                                        float* __restrict__ xa2, float* __restrict__ xb2,
                                                        real* __restrict__ ua2, real* __restrict__ ub2,
                                                        const real* __restrict__ x0, real* __restrict__ x02,
                                                        const real* __restrict__ Jn, real* __restrict__ Jn2,
                                                        const int* __restrict__ rs, int* __restrict__ rs2,
                                                        const int* __restrict__ orig, int* __restrict__ orig2,
                                                        const int* __restrict__ ntr, int* __restrict__ ntr2) {
    const int slot = blockIdx.x, lane = threadIdx.x, j = slot * TILE + lane;
    const bool valid = j < count;
    int tile, hl;
    ls_locate(sc, ntiles_old, valid ? j : count - 1, tile, hl);
    const int t_lo = blockIdx.y * LS_GCH;
    const int t_hi = t_lo + LS_GCH < T ? t_lo + LS_GCH : T;
    for (int t = t_lo; t < t_hi; t++) {
        float a[6], b[6];
        real c[2], d[2];
#pragma unroll
        for (int i = 0; i < 6; i++) { a[i] = xa[tix<6>(tile, T, t, i, hl)]; b[i] = xb[tix<6>(tile, T, t, i, hl)]; }
#pragma unroll
        for (int i = 0; i < 2; i++) { c[i] = ua[tix<2>(tile, T, t, i, hl)]; d[i] = ub[tix<2>(tile, T, t, i, hl)]; }
#pragma unroll
        for (int i = 0; i < 6; i++) { xa2[tix<6>(slot, T, t, i, lane)] = a[i]; xb2[tix<6>(slot, T, t, i, lane)] = b[i]; }
#pragma unroll
        for (int i = 0; i < 2; i++) { ua2[tix<2>(slot, T, t, i, lane)] = c[i]; ub2[tix<2>(slot, T, t, i, lane)] = d[i]; }
    }
    if (blockIdx.y == 0) {
        const int b = tile * TILE + hl;
#pragma unroll
        for (int i = 0; i < 6; i++) x02[((size_t)slot * 6 + i) * TILE + lane] = x0[((size_t)tile * 6 + i) * TILE + hl];
        Jn2[j] = Jn[b];
        rs2[j] = rs[b];
        orig2[j] = valid ? orig[b] : -1;
        ntr2[j] = ntr[b];      // the trial count of the last search: the scheduling hint of the next one
    }
}

struct SolveWs {
    void* newton;
    float* xw[4];
    real* uw[4];
    real* J[2][2];
    real* x0g[2];
    int* run_status[2];
    int* orig[2];
    int* ntrials[2];
    real *descent, *stepsize;
    int* n_active;
    int* code;
    unsigned long long* mask;
    int* prefix;
};

static size_t solve_ws_carve(int32_t B, int32_t T, void* base, SolveWs* w) {
    const size_t nt = (size_t)aoc_ntiles(B), Bp = nt * TILE;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return base ? (char*)base + o : (char*)nullptr; };
    char* q = take(api_workspace_bytes_upto(B, T));
    if (w) w->newton = q;
    for (int i = 0; i < 4; i++) { q = take(aoc_tiled_elems(B, T, 6) * sizeof(float)); if (w) w->xw[i] = (float*)q; }
    for (int i = 0; i < 4; i++) { q = take(aoc_tiled_elems(B, T, 2) * sizeof(real)); if (w) w->uw[i] = (real*)q; }
    for (int g = 0; g < 2; g++) {
        for (int i = 0; i < 2; i++) { q = take(Bp * sizeof(real)); if (w) w->J[g][i] = (real*)q; }
        q = take(Bp * 6 * sizeof(real)); if (w) w->x0g[g] = (real*)q;
        q = take(Bp * sizeof(int)); if (w) w->run_status[g] = (int*)q;
        q = take(Bp * sizeof(int)); if (w) w->orig[g] = (int*)q;
        q = take(Bp * sizeof(int)); if (w) w->ntrials[g] = (int*)q;
    }
    q = take(Bp * sizeof(real)); if (w) w->descent = (real*)q;
    q = take(Bp * sizeof(real)); if (w) w->stepsize = (real*)q;
    q = take(Bp * sizeof(int)); if (w) w->code = (int*)q;
    q = take(nt * sizeof(unsigned long long)); if (w) w->mask = (unsigned long long*)q;
    q = take((nt + 1) * sizeof(int)); if (w) w->prefix = (int*)q;
    q = take(256); if (w) w->n_active = (int*)q;
    return off;
}

// how aoc_newton_solve cuts a batch in two when it is given a second stream: by tiles, the first half rounded down
static int solve_split_tiles_a(int32_t B) { return aoc_ntiles(B) / 2; }
static bool solve_splits(int32_t B) { return aoc_ntiles(B) >= tuning().solve_split_tiles && aoc_ntiles(B) >= 2; }

// The workspace serves the whole batch as one part, or its two halves side by side — whichever is larger — so that the
// caller sizes it once, second stream or not.
static size_t api_solve_workspace_bytes(int32_t B, int32_t T) {
    const size_t one = solve_ws_carve(B, T, nullptr, nullptr);
    if (aoc_ntiles(B) < 2) return one;
    const int Ba = solve_split_tiles_a(B) * TILE;
    const size_t two = solve_ws_carve(Ba, T, nullptr, nullptr) + solve_ws_carve(B - Ba, T, nullptr, nullptr);
    return one > two ? one : two;
}

// One part of a solve (the whole batch, or one of its halves on a stream of its own) as a resumable sequence:
// begin() | { enqueue() -> a count is on its way | resume(): blocks for it, stops or re-packs } ... | finish().
// aoc_newton_solve drives one or two of these from one host thread: while it waits for one part's counter the other
// part's launches are already queued on the other stream.
struct SolveRun {
    aoc_problem base;          // this part's problem: B, stream, ref
    const aoc_params* prm;
    const void* x_init; const real* u_init; const real* x0;
    void* x_star; real* u_star;
    int32_t *iters, *ret_index, *status;
    real *h_cost, *h_desc, *h_step; int32_t* h_ntr;
    int hstride, sync_every, part;
    SolveWs w;
    size_t newton_bytes;
    hipStream_t st;
    int nt0, T, n_it, repack_off;
    int nt_caller;             // tiles of the caller's whole batch: what the horizon cut is decided on for every generation and half
    // state
    SolveGen g;
    int gen, kk, last, next_sync, interval, absorbed;
    bool pending, done;
    // diagnostic timeline
    bool tracing;
    std::vector<hipEvent_t> tev;
    std::vector<int> t_b, t_left, t_kk;

    void trace_mark(int kk_) {
        if (!tracing) return;
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, st);
        tev.push_back(e); t_b.push_back(g.B); t_left.push_back(-1); t_kk.push_back(kk_);
    }
    const void* xsrc(int i) const { return i == 0 ? x_init : (const void*)g.x[(i - 1) % 3]; }
    const real* usrc(int i) const { return i == 0 ? u_init : (const real*)g.u[(i - 1) % 3]; }

    void book(int kk_, int final_pass, int src_iter) {
        const bool have = src_iter >= 0;
        const bool src_f32 = src_iter == 0 ? base.x_in_f32 != 0 : true;
        const void* xs = have ? xsrc(src_iter) : nullptr;
        const real* us = have ? usrc(src_iter) : nullptr;
        const int ntg = aoc_ntiles(g.B);
        const float* xn = final_pass ? nullptr : g.x[kk_ % 3];     // iterate kk+1
        const real* un = final_pass ? nullptr : g.u[kk_ % 3];
        hipLaunchKernelGGL(k_solve_book, dim3(ntg), dim3(TILE), 0, st, T, kk_, (real)prm->term_cond, final_pass, n_it, g.orig,
                           w.descent, g.J[kk_ & 1], w.stepsize, w.ntrials[gen & 1], g.run_status, ret_index, iters, status,
                           w.n_active, have ? 1 : 0, un, w.code, h_cost, h_desc, h_step, h_ntr, hstride);
        AOC_DISPATCH_XT(src_f32, XS, AOC_DISPATCH_XT(base.x_out_f32, XO,
            hipLaunchKernelGGL((k_solve_copy<XS, XO>), dim3(ntg, SOLVE_COPY_NY), dim3(TILE), 0, st, T, src_iter == 0 ? 1 : 0,
                               g.orig, w.code, (const XS*)xs, us, un, (XO*)x_star, u_star)));
        (void)xn;
    }

    int begin() {
        st = (hipStream_t)base.stream;
        nt0 = aoc_ntiles(base.B); T = base.T;
        n_it = prm->max_iters - 1 > 0 ? prm->max_iters - 1 : 0;
        // per-trajectory reference curves stay where the caller put them (lane b reads curve b): such a batch is never
        // re-packed (round 3 re-packed it and read the wrong curves afterwards; tests/test_gpu_parity.py two-manoeuvre case)
        repack_off = tuning().solve_norepack || base.ref_per_traj;
        for (int i = 0; i < 3; i++) { g.x[i] = w.xw[i]; g.u[i] = w.uw[i]; }
        g.xs = w.xw[3]; g.us = w.uw[3];
        g.x0 = x0; g.J[0] = w.J[0][0]; g.J[1] = w.J[0][1]; g.run_status = w.run_status[0]; g.orig = w.orig[0]; g.B = base.B;
        gen = 0; kk = 0; last = -1; absorbed = 0; pending = false; done = n_it == 0;
        interval = sync_every; next_sync = sync_every > 0 ? sync_every - 1 : -1;
        hipLaunchKernelGGL(k_solve_init, dim3(nt0), dim3(TILE), 0, st, base.B, ret_index, iters, status, g.run_status, g.orig,
                           w.n_active);
        // the line search reads the previous iteration's trial counts as a scheduling hint: none before the first iteration
        if (hipMemsetAsync(w.ntrials[0], 0, (size_t)nt0 * TILE * sizeof(int), st) != hipSuccess) return check_launch("aoc_newton_solve");
        aoc_problem pi = base;
        pi.x_out_f32 = 1;
        const int rc = api_traj_cost(&pi, x_init, u_init, x0, g.J[0]);
        trace_mark(-1);
        return rc;
    }

    // launches iterations up to and including the next sync point; pending = a count read is due (resume())
    int enqueue() {
        while (!done) {
            aoc_problem pi = base;
            pi.x_out_f32 = 1;
            pi.B = g.B;
            pi.x_in_f32 = kk == 0 ? base.x_in_f32 : 1;
            pi.x_is_rollout = kk == 0 ? base.x_is_rollout : 1;   // every later iterate was written by the line search's rollout
            const int rc = api_newton_iterate(&pi, prm, kk, xsrc(kk), usrc(kk), g.x0, g.J[kk & 1], w.newton, newton_bytes,
                                              g.x[kk % 3], g.u[kk % 3], g.J[(kk + 1) & 1], w.descent, w.stepsize,
                                              w.ntrials[gen & 1], g.run_status, LsFrozen{g.orig, ret_index}, nt_caller);
            if (rc) return rc;
            last = kk;
            book(kk, 0, kk - 1);
            trace_mark(kk);
            const bool sync_now = sync_every > 0 && kk == next_sync && kk < n_it - 1;
            kk++;
            if (kk >= n_it) done = true;
            if (sync_now) { pending = true; return AOC_OK; }
        }
        return AOC_OK;
    }

    // the host's look at the counter: stop when nobody iterates, re-pack when few do
    int resume() {
        if (!pending) return AOC_OK;
        pending = false;
        int cnt[2] = {0, 0};
        if (hipMemcpyAsync(cnt, w.n_active, sizeof cnt, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return check_launch("aoc_newton_solve");
        const int left = cnt[0];
        absorbed = cnt[1];
        if (tracing && !t_left.empty()) t_left.back() = left;
        if (left == 0) { done = true; return AOC_OK; }
        const int kd = kk - 1;               // the iteration just completed
        // once trajectories stop, look more often: the count then falls by 15-30 % per iteration
        const int fast = tuning().solve_sync_fast > 0 ? tuning().solve_sync_fast : 1;
        if (left < base.B && fast < interval) interval = fast;
        next_sync = kd + interval;
        // re-pack: the newest iterate (kd+1) of the `left` iterating trajectories goes into the free slot, the one before
        // it (kd) into the spare
        const int fs = (kd + 1) % 3, ns = kd % 3, ps = (kd + 2) % 3;   // free, newest, previous
        const int nt_new = (left + TILE - 1) / TILE;
        if (!repack_off && kd >= 1 && g.B > SOLVE_REPACK_MIN && (long)left * 100 <= (long)g.B * tuning().solve_repack_pct &&
            nt_new < aoc_ntiles(g.B)) {
            const int ntg = aoc_ntiles(g.B), ng = gen + 1;
            LsScratch sc;
            memset(&sc, 0, sizeof sc);
            sc.mask = w.mask; sc.prefix = w.prefix;
            hipLaunchKernelGGL(k_repack_mask, dim3(ntg), dim3(TILE), 0, st, g.orig, ret_index, w.mask);
            hipLaunchKernelGGL(k_prefix_popc, dim3(1), dim3(1024), 0, st, ntg, w.mask, w.prefix);
            SolveGen h = g;
            h.x[ns] = g.x[fs];  h.u[ns] = g.u[fs];
            h.x[ps] = g.xs;     h.u[ps] = g.us;
            h.x[fs] = g.x[ns];  h.u[fs] = g.u[ns];
            h.xs = g.x[ps];     h.us = g.u[ps];
            h.x0 = w.x0g[ng & 1];
            h.J[0] = w.J[ng & 1][0]; h.J[1] = w.J[ng & 1][1];
            h.run_status = w.run_status[ng & 1]; h.orig = w.orig[ng & 1];
            h.B = left;
            hipLaunchKernelGGL(k_repack_gather, dim3(nt_new, (T + LS_GCH - 1) / LS_GCH), dim3(TILE), 0, st, T, ntg, left,
                               sc, (const float*)g.x[ns], (const float*)g.x[ps], (const real*)g.u[ns],
                               (const real*)g.u[ps], h.x[ns], h.x[ps], h.u[ns], h.u[ps], g.x0, (real*)h.x0,
                               (const real*)g.J[(kd + 1) & 1], h.J[(kd + 1) & 1], (const int*)g.run_status,
                               h.run_status, (const int*)g.orig, h.orig, (const int*)w.ntrials[gen & 1], w.ntrials[ng & 1]);
            g = h;
            gen = ng;
        }
        return AOC_OK;
    }

    int finish() {
        book(last, 1, last + 1);     // last = -1 (max_iters <= 1): everybody returns the initial iterate, index 0
        {   // the states of every returned iterate of index >= 1: one rollout of its inputs (see solve_copy_out)
            aoc_problem pb = base;
            KConst kc = make_const(&pb);
            AOC_DISPATCH_XT(base.x_out_f32, XO,
                hipLaunchKernelGGL((k_solve_restate<XO>), dim3(nt0), dim3(TILE), 0, st, kc, (const int*)ret_index, x0, (const real*)u_star,
                                   (XO*)x_star));
        }
        trace_mark(last + 1);
        return AOC_OK;
    }
};

static int api_newton_solve(const aoc_problem* p, const aoc_params* prm, const void* x_init, const real* u_init,
                            const real* x0, void* workspace, size_t workspace_bytes, int32_t sync_every, void* x_star, real* u_star,
                            int32_t* iters, int32_t* ret_index, int32_t* status, real* h_cost, real* h_desc,
                            real* h_step, int32_t* h_ntr, int32_t* n_run, void* stream2) {
    int rc = check_problem(p);
    if (!rc) rc = check_riccati_weights(p, stream2 ? "aoc_newton_solve2" : "aoc_newton_solve");
    if (rc) return rc;
    if (!prm || !x_init || !u_init || !x0 || !workspace || !x_star || !u_star || !iters || !ret_index || !status)
        return AOC_EINVAL;
    if (sizeof(real) != 8) return AOC_EINVAL;  // the solve level is the parity (fp64) path
    if (workspace_bytes < api_solve_workspace_bytes(p->B, p->T))
        return einval("aoc_newton_solve: workspace of %zu bytes, %zu needed (aoc_solve_workspace_bytes)", workspace_bytes,
                      api_solve_workspace_bytes(p->B, p->T));
    hipStream_t st1 = (hipStream_t)p->stream;
    const int nt0 = aoc_ntiles(p->B), Bp0 = nt0 * TILE, T = p->T;
    const int n_it = prm->max_iters - 1 > 0 ? prm->max_iters - 1 : 0;
    if (n_it > 0 && (h_cost || h_desc || h_step || h_ntr)) {
        const size_t n = (size_t)n_it * Bp0;
        hipLaunchKernelGGL(k_solve_hist_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st1, n, h_cost, h_desc, h_step,
                           h_ntr);
    }
    // one part, or two halves (cut by tiles) on two streams that never wait for each other
    const bool two = stream2 != nullptr && (hipStream_t)stream2 != st1 && solve_splits(p->B);
    const int nparts = two ? 2 : 1;
    SolveRun run[2];
    const int nta = two ? solve_split_tiles_a(p->B) : nt0;
    char* wsp = (char*)workspace;
    for (int i = 0; i < nparts; i++) {
        SolveRun& r = run[i];
        const size_t t0 = i == 0 ? 0 : (size_t)nta;          // first tile of the part
        const size_t b0 = t0 * TILE;
        r.base = *p;
        r.base.B = two ? (i == 0 ? nta * TILE : p->B - nta * TILE) : p->B;
        r.base.stream = i == 0 ? p->stream : stream2;
        if (p->ref_per_traj)
            r.base.ref = (const char*)p->ref + t0 * (size_t)(p->ref_T ? p->ref_T : T) * 8 * TILE * sizeof(real);
        r.prm = prm;
        r.x_init = (const char*)x_init + t0 * T * 6 * TILE * (p->x_in_f32 ? sizeof(float) : sizeof(real));
        r.u_init = u_init + t0 * T * 2 * TILE;
        r.x0 = x0 + t0 * 6 * TILE;
        r.x_star = (char*)x_star + t0 * T * 6 * TILE * (p->x_out_f32 ? sizeof(float) : sizeof(real));
        r.u_star = u_star + t0 * T * 2 * TILE;
        r.iters = iters + b0; r.ret_index = ret_index + b0; r.status = status + b0;
        r.h_cost = h_cost ? h_cost + b0 : nullptr; r.h_desc = h_desc ? h_desc + b0 : nullptr;
        r.h_step = h_step ? h_step + b0 : nullptr; r.h_ntr = h_ntr ? h_ntr + b0 : nullptr;
        r.hstride = Bp0; r.sync_every = sync_every; r.part = i; r.nt_caller = nt0;
        wsp += solve_ws_carve(r.base.B, T, wsp, &r.w);
        r.newton_bytes = api_workspace_bytes_upto(r.base.B, T);   // every generation iterates in the first one's workspace
        r.tracing = g_solve_trace.rows != nullptr;
    }
    hipEvent_t fork = nullptr, join = nullptr;
    if (two) {   // the second stream starts after what the caller queued on the first ...
        if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) return check_launch("aoc_newton_solve");
        if (hipEventCreateWithFlags(&join, hipEventDisableTiming) != hipSuccess) {
            (void)hipEventDestroy(fork);
            return check_launch("aoc_newton_solve");
        }
        (void)hipEventRecord(fork, st1);
        (void)hipStreamWaitEvent((hipStream_t)stream2, fork, 0);
    }
    auto cleanup = [&] {
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        for (int i = 0; i < nparts; i++)
            for (hipEvent_t e : run[i].tev) (void)hipEventDestroy(e);
    };
    for (int i = 0; i < nparts && !rc; i++) rc = run[i].begin();
    for (int i = 0; i < nparts && !rc; i++) rc = run[i].enqueue();
    while (!rc) {
        bool any = false;
        for (int i = 0; i < nparts && !rc; i++) {
            if (!run[i].pending) continue;
            any = true;
            rc = run[i].resume();
            if (!rc) rc = run[i].enqueue();
        }
        if (!any) break;
    }
    if (rc) {   // work already queued on either stream may still use the workspace and the caller's arrays: a caller who
        //       frees them on error must not race with it
        (void)hipStreamSynchronize(st1);
        if (two) (void)hipStreamSynchronize((hipStream_t)stream2);
        cleanup();
        return rc;
    }
    int nr = 0;
    for (int i = 0; i < nparts; i++) {
        run[i].finish();
        // a retired all-NaN trajectory stands for iterations up to max_iters-1 (see above)
        const int r_i = run[i].absorbed > 0 || run[i].sync_every <= 0 ? run[i].n_it : run[i].last + 1;
        if (r_i > nr) nr = r_i;
    }
    if (two) {   // ... and the first stream continues after both
        (void)hipEventRecord(join, (hipStream_t)stream2);
        (void)hipStreamWaitEvent(st1, join, 0);
    }
    if (n_run) *n_run = nr;
    if (g_solve_trace.rows) {
        g_solve_trace.n = 0;
        for (int i = 0; i < nparts; i++)
            if (!run[i].tev.empty()) (void)hipEventSynchronize(run[i].tev.back());
        for (int i = 0; i < nparts; i++) {
            SolveRun& r = run[i];
            for (size_t j = 1; j < r.tev.size() && g_solve_trace.n < g_solve_trace.cap; j++) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, run[0].tev[0], r.tev[j]);
                double* row = g_solve_trace.rows + (size_t)g_solve_trace.n++ * SOLVE_TRACE_COLS;
                row[0] = i; row[1] = r.t_kk[j]; row[2] = r.t_b[j]; row[3] = aoc_ntiles(r.t_b[j]); row[4] = r.t_left[j]; row[5] = ms;
            }
        }
    }
    cleanup();
    return check_launch("aoc_newton_solve");
}


// One receding-horizon step for every instance (see include/aoc.h: aoc_mpc_step).
static int api_mpc_step(const aoc_problem* p_track, const aoc_problem* p_next, const aoc_params* prm, int32_t n_newton,
                        const void* x_cur, const real* u_cur, real* x0, real* x_true, const real* disturbance,
                        void* workspace, size_t workspace_bytes, real* Kgain, void* x_a, real* u_a, void* x_b, real* u_b, real* J_a, real* J_b,
                        real* descent, real* stepsize, int32_t* ntrials, int32_t* status, real* K0, real* u_applied,
                        int32_t* final_slot, const aoc_mpc_noise* noise = nullptr, real* disturbance_out = nullptr) {
    int rc = check_problem(p_track);
    if (!rc) rc = check_riccati_weights(p_track, "aoc_mpc_step (p_track)");
    if (rc) return rc;
    rc = check_problem(p_next);
    if (!rc) rc = check_riccati_weights(p_next, "aoc_mpc_step (p_next)");
    if (rc) return rc;
    if (p_track->B != p_next->B || p_track->T != p_next->T || p_next->T < 3) return AOC_EINVAL;
    if (!prm || n_newton < 0 || !x_cur || !u_cur || !x0 || !x_true || !workspace || !Kgain || !x_a || !u_a || !x_b || !u_b ||
        !J_a || !J_b || !descent || !stepsize || !ntrials || !u_applied)
        return AOC_EINVAL;
    if (!p_track->x_in_f32 || !p_next->x_in_f32 || !p_next->x_out_f32) return AOC_EINVAL;  // float32 state buffers throughout
    hipStream_t st = (hipStream_t)p_next->stream;
    // 1. gains about the current optimum (weights of p_track)
    rc = api_lqr_tracking(p_track, x_cur, u_cur, x0, nullptr, Kgain, nullptr, nullptr, status, workspace, workspace_bytes);   // the workspace is free until the first iteration
    if (rc) return rc;
    // 2. closed-loop plant step, x0 <- new plant state; 3. inputs shifted by one sample; 4. warm start: their rollout from
    //    the new x0 into buffer a.  Small batches: one launch (k_mpc_warm_split); otherwise three (the shifted inputs go
    //    through buffer b, free until the first iteration writes it)
    KConst k = make_const(p_next);
    MpcNoise nz;
    memset(&nz, 0, sizeof nz);
    if (noise) {
        nz.key0 = (unsigned)(noise->seed & 0xffffffffull); nz.key1 = (unsigned)(noise->seed >> 32);
        nz.step = noise->step; nz.first = noise->first;
        for (int c = 0; c < 6; c++) nz.sigma[c] = noise->sigma[c];
        nz.on = 1;
    }
    if (k.ntiles <= tuning().split_tiles) {
        AOC_DISPATCH_DR(k, D, RP,
            hipLaunchKernelGGL((k_mpc_warm_split<D, RP, float>), dim3(k.ntiles), dim3(2 * TILE), 0, st, k, (const real*)p_next->ref,
                               (const real*)Kgain, u_cur, x0, x_true, disturbance, K0, u_applied, (float*)x_a, u_a, J_a, status, nz,
                               disturbance_out));
    } else {
        hipLaunchKernelGGL(k_mpc_advance, dim3(k.ntiles), dim3(TILE), 0, st, k, (const real*)Kgain, u_cur, x0, x_true, disturbance,
                           K0, u_applied, nz, disturbance_out);
        hipLaunchKernelGGL(k_shift_inputs, dim3(k.ntiles, p_next->T < 64 ? p_next->T : 64), dim3(TILE), 0, st, p_next->T, u_cur, u_b);
        rc = api_rollout_cost(p_next, x0, u_b, nullptr, nullptr, x_a, u_a, J_a, status);
        if (rc) return rc;
    }
    // 5. re-solve: kk restarts at 0 (Gauss-Newton Hessian only, Q4); iterates alternate between the two buffers
    void* xs[2] = {x_a, x_b};
    real* us[2] = {u_a, u_b};
    real* Js[2] = {J_a, J_b};
    int cur = 0;
    aoc_problem pn = *p_next;
    pn.x_is_rollout = 1;   // the warm start and every later iterate are rollouts of their inputs
    for (int kk = 0; kk < n_newton; kk++) {
        rc = api_newton_iterate(&pn, prm, kk, xs[cur], us[cur], x0, Js[cur], workspace, workspace_bytes, xs[1 - cur], us[1 - cur],
                                Js[1 - cur], descent, stepsize, ntrials, status);
        if (rc) return rc;
        cur = 1 - cur;
    }
    if (final_slot) *final_slot = cur;
    return check_launch("aoc_mpc_step");
}

