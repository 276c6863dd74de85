// passes/api.inc — launch functions: the bodies of the C-ABI entry points of include/aoc.h.
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// launch functions (bodies of the C-ABI entry points of include/aoc.h, arrays typed `real`)
// ---------------------------------------------------------------------------------------------
static KConst make_const(const aoc_model& md, const double* Q, const double* R, const double* QT, int B, int T) {
    KConst k;
    memset(&k, 0, sizeof k);
    k.cd0 = (real)md.cd0; k.cda = (real)md.cda; k.cla = (real)md.cla; k.m = (real)md.m; k.g = (real)md.g; k.S = (real)md.S;
    k.rho = (real)md.rho;
    k.J = (real)md.J; k.dt = (real)md.dt;
    k.dtm = (real)(md.dt / md.m);
    k.mg = (real)(md.m * md.g);
    k.hrho = (real)(0.5 * md.rho);
    k.krs = (real)(md.rho * md.S);
    k.b41 = (real)(md.dt / md.J);
    k.rJ = R(1.0) / k.J;
    for (int i = 0; i < 36; i++) { if (Q) k.Q[i] = (real)Q[i]; if (QT) k.QT[i] = (real)QT[i]; }
    for (int i = 0; i < 4; i++) if (R) k.R[i] = (real)R[i];
    k.B = B; k.T = T; k.ntiles = (B + TILE - 1) / TILE;
    k.refT = T; k.rpt = 0;
    k.diag = (Q && R && QT) ? (is_diag(Q, 6) && is_diag(R, 2) && is_diag(QT, 6)) : 1;
    return k;
}

static KConst make_const(const aoc_problem* p) {
    KConst k = make_const(p->model, p->QQt, p->RRt, p->QQT, p->B, p->T);
    k.rpt = p->ref_per_traj != 0;
    if (k.rpt && p->ref_T > 0) k.refT = p->ref_T;
    return k;
}

static int api_step_batch(const aoc_model* model, int32_t n, const real* x, const real* u, const real* lmbd,
                   real* xp, real* fx, real* fu, real* fxx, real* fuu, real* fux, void* stream) {
    if (!model || !x || !u || !xp || n < 1) return AOC_EINVAL;
    KConst k = make_const(*model, nullptr, nullptr, nullptr, n, 3);
    hipLaunchKernelGGL(k_step_batch, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, k, n, x, u, lmbd, xp,
                       fx, fu, fxx, fuu, fux);
    return check_launch("k_step_batch");
}

static int api_cost_batch(const aoc_problem* prob, int32_t n, const real* x, const real* u, const real* xr,
                   const real* ur, real* ll, real* lx, real* lu, real* llT, real* lTx, void* stream) {
    if (!prob || !x || !u || !xr || !ur || n < 1) return AOC_EINVAL;
    KConst k = make_const(prob->model, prob->QQt, prob->RRt, prob->QQT, n, 3);
    if (k.diag)
        hipLaunchKernelGGL(k_cost_batch<true>, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, k, n, x, u, xr,
                           ur, ll, lx, lu, llT, lTx);
    else
        hipLaunchKernelGGL(k_cost_batch<false>, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, k, n, x, u, xr,
                           ur, ll, lx, lu, llT, lTx);
    return check_launch("k_cost_batch");
}

static int api_traj_cost(const aoc_problem* p, const void* x, const real* u, const real* x0, real* J) {
    int rc = check_problem(p);
    if (rc) return rc;
    if (!x || !u || !x0 || !J) return AOC_EINVAL;
    KConst k = make_const(p);
    hipStream_t st = (hipStream_t)p->stream;
    AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,
        hipLaunchKernelGGL((k_traj_cost<D, RP, XT>), dim3(k.ntiles), dim3(TILE), 0, st, k, (const real*)p->ref, (const XT*)x, u, x0, J)));
    return check_launch("k_traj_cost");
}

static int api_initial_trajectory(const aoc_problem* p, real kp, real kt, const real* x0, void* x, real* u) {
    int rc = check_problem(p);
    if (rc) return rc;
    if (!x0 || !x || !u) return AOC_EINVAL;
    KConst k = make_const(p);
    AOC_DISPATCH_RPT(k.rpt, RP, AOC_DISPATCH_XT(p->x_out_f32, XO,
        hipLaunchKernelGGL((k_initial_traj<RP, XO>), dim3(k.ntiles), dim3(TILE), 0, (hipStream_t)p->stream, k, kp, kt,
                           (const real*)p->ref, x0, (XO*)x, u)));
    return check_launch("k_initial_traj");
}

static int api_rollout_cost(const aoc_problem* p, const real* x0, const real* u, const real* du,
                     const real* alpha, void* x_out, real* u_out, real* J_out, int32_t* status) {
    int rc = check_problem(p);
    if (rc) return rc;
    if (!x0 || !u || !J_out) return AOC_EINVAL;
    if ((x_out == nullptr) != (u_out == nullptr)) return AOC_EINVAL;
    if (du && !alpha) return AOC_EINVAL;
    KConst k = make_const(p);
    hipStream_t st = (hipStream_t)p->stream;
    const int split_tiles = tuning().split_tiles;
    if (x_out && k.ntiles <= split_tiles && p->T >= 3) {
        AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_out_f32, XO,
            hipLaunchKernelGGL((k_rollout_cost_split<D, RP, XO>), dim3(k.ntiles), dim3(2 * TILE), 0, st, k, (const real*)p->ref, x0,
                               u, du, alpha, (XO*)x_out, u_out, J_out, status)));
        return check_launch("k_rollout_cost");
    }
    AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_BOOL(x_out != nullptr, W, AOC_DISPATCH_XT(p->x_out_f32, XO,
        hipLaunchKernelGGL((k_rollout_cost<D, RP, W, XO>), dim3(k.ntiles), dim3(TILE), 0, st, k, (const real*)p->ref, x0, u, du, alpha,
                           (XO*)x_out, u_out, J_out, status))));
    return check_launch("k_rollout_cost");
}

// the boundary value functions of a cut pass: the chain of hops, by default through pairwise composed maps (k_hcut_pair,
// k_hcut_odd: aoc_tuning.hcut_pairs), or the several-wavefront form of the plain chain (aoc_tuning.hcut_chain6)
template <bool AFFINE>
static void hcut_launch_chain(int ntiles, int S, real* scratch, hipStream_t st) {
    if (tuning().hcut_chain6) {
        hipLaunchKernelGGL(k_hcut_chain6<AFFINE>, dim3(ntiles), dim3(4 * TILE), 0, st, S, scratch);
        return;
    }
    // worth it from about a dozen segments on (16: chain 14 -> 7 hops, -17 us of 65; 8 segments, the cut of 65-128 tiles:
    // 6 -> 3 hops buys less than the two extra launches cost, +2 % per iteration); the knob's 2 composes whenever it can
    const int np = (tuning().hcut_pairs >= 2 || (tuning().hcut_pairs == 1 && S >= 12)) ? hcut_npairs(S) : 0;
    if (np) hipLaunchKernelGGL(k_hcut_pair<AFFINE>, dim3(ntiles, np), dim3(2 * TILE), 0, st, S, scratch);
    hipLaunchKernelGGL(k_track_hcut_chain<AFFINE>, dim3(ntiles), dim3(TILE), 0, st, S, scratch, np);
    if (np) hipLaunchKernelGGL(k_hcut_odd<AFFINE>, dim3(ntiles, np), dim3(TILE), 0, st, S, scratch);
}

// Is a pass cut, and how: the one place that decides it.  kind: the Gauss-Newton or full-Hessian backward pass of the Newton
// iteration, or the tracking gains; knob: that pass's number of segments (aoc_tuning.bw_hcut / track_hcut); decide_ntiles: the
// tile count the number of segments is chosen on, ntiles: the batch in flight.  S and bytes describe the cut the knob asks
// for (aoc_backward_scratch_bytes sizes by them); `cut` says whether this pass takes it: at least two segments of at least
// four stages, a grid of at most 1024 workgroups, scratch of `bytes`, fp64.
enum HcutKind { HCUT_GN, HCUT_FULL, HCUT_TRACK };
struct HcutPlan { int S; bool multiwave; size_t bytes; bool cut; };
static HcutPlan hcut_plan(HcutKind kind, int knob, int decide_ntiles, int ntiles, int T, const void* scratch, size_t scratch_bytes) {
    HcutPlan pl;
    pl.S = hcut_segments(knob, decide_ntiles, kind == HCUT_FULL);
    pl.multiwave = hcut_multiwave(tuning().hcut_waves, ntiles, pl.S);   // (scheduling only: bit-identical either way)
    pl.bytes = pl.S < 2 ? 0 : kind == HCUT_FULL ? hcut_full_scratch_bytes(ntiles, pl.S) : hcut_scratch_bytes(ntiles, pl.S);
    pl.cut = pl.S >= 2 && scratch && sizeof(real) == 8 && ntiles * pl.S <= 1024 && T - 1 >= 4 * pl.S && pl.bytes <= scratch_bytes;
    return pl;
}

// The cut backward pass of the Newton iteration, Gauss-Newton or FULL Hessian: segment maps -> chain -> gains, on one or on
// several wavefronts per (tile, segment).  FULL: the costate maps first, and at the end the sequential kernel for the tiles
// the cut does not trust (round 5).
template <bool FULL>
static void hcut_launch_backward(const aoc_problem* p, const KConst& k, const HcutPlan& pl, const void* x, const real* u,
                                 const real* x0, real* Kt, int32_t* status, void* scratch, hipStream_t st) {
    const int S = pl.S;
    HcutFull hf{nullptr, nullptr, nullptr, nullptr, 0};
    if (FULL) {
        hf = hcut_full_carve(scratch, k.ntiles, S);
        hf.trust = tuning().bw_hcut_full >= 2;
    }
#define LAUNCH_HC(KERNEL, NY, NW, ...)                                                                                 \
    AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,                                                       \
        hipLaunchKernelGGL(KERNEL, dim3(k.ntiles, NY), dim3((NW) * TILE), 0, st, k, S, (const real*)p->ref, (const XT*)x, u, x0, __VA_ARGS__)))
    if (FULL) LAUNCH_HC((k_bw_hcut_lam<D, RP, XT>), S, 1, hf);
    if (pl.multiwave) LAUNCH_HC((k_bw_hcut_map3<D, RP, XT, FULL>), S, 3, Kt, (real*)scratch, status, hf);
    else LAUNCH_HC((k_bw_hcut<D, RP, XT, false, FULL>), S, 1, Kt, (real*)scratch, status, hf);
    hcut_launch_chain<true>(k.ntiles, S, (real*)scratch, st);
    if (pl.multiwave) LAUNCH_HC((k_bw_hcut_gains2<D, RP, XT, FULL>), S - 1, 2, Kt, (real*)scratch, status, hf);
    else LAUNCH_HC((k_bw_hcut<D, RP, XT, true, FULL>), S - 1, 1, Kt, (real*)scratch, status, hf);
#undef LAUNCH_HC
    if (FULL)
        AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,
            hipLaunchKernelGGL((k_backward2<D, RP, true, true, XT>), dim3(k.ntiles), dim3(2 * TILE), 0, st, k, (const real*)p->ref,
                               (const XT*)x, u, x0, Kt, (real*)nullptr, status, (const int*)hf.tile_flag, (const int*)hf.lane_flags)));
}

// hcut_ntiles: the tile count the horizon cut is decided on (0 = this batch's own).  aoc_newton_solve passes the tile count
// of the CALLER's batch for every generation and half, so that a trajectory's bits do not depend on the batch it happens
// to be solved in (re-packing and the two-stream split are scheduling only).
static int api_backward(const aoc_problem* p, int32_t full_hessian, const void* x, const real* u, const real* x0,
                 real* Kt, real* lmbd0, int32_t* status, void* scratch = nullptr, size_t scratch_bytes = 0, int hcut_ntiles = 0) {
    int rc = check_problem(p);
    if (!rc) rc = check_riccati_weights(p, "aoc_backward");
    if (rc) return rc;
    if (!x || !u || !x0 || !Kt) return AOC_EINVAL;
    KConst k = make_const(p);
    hipStream_t st = (hipStream_t)p->stream;
    const bool lam = full_hessian != 0 || lmbd0 != nullptr;
    // batches that leave most SIMDs idle: the horizon in S segments (k_bw_hcut) — Gauss-Newton iterations, and full-Hessian
    // ones (aoc_tuning.bw_hcut_full)
    const bool cut_full = full_hessian && !lmbd0 && tuning().bw_hcut_full;
    if (!lam || cut_full) {
        const HcutPlan pl = hcut_plan(cut_full ? HCUT_FULL : HCUT_GN, tuning().bw_hcut, hcut_ntiles > 0 ? hcut_ntiles : k.ntiles,
                                      k.ntiles, p->T, scratch, scratch_bytes);
        if (pl.cut) {
            if (cut_full) hcut_launch_backward<true>(p, k, pl, x, u, x0, Kt, status, scratch, st);
            else hcut_launch_backward<false>(p, k, pl, x, u, x0, Kt, status, scratch, st);
            return check_launch(cut_full ? "k_bw_hcut (full Hessian)" : "k_bw_hcut");
        }
    }
#define LAUNCH_BW(F, L)                                                                                        \
    AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,                                              \
        hipLaunchKernelGGL((k_backward<D, RP, F, L, XT>), dim3(k.ntiles), dim3(TILE), 0, st, k, (const real*)p->ref, \
                           (const XT*)x, u, x0, Kt, lmbd0, status)))
    // small batches (at most one tile per two SIMDs): two wavefronts per tile, see k_backward2.  Measured per
    // iteration of the backward pass: 4096 trajectories 0.85 -> 0.54 ms, 32 768 1.05 -> 0.78.  Beyond 512 tiles the
    // pass itself still gets shorter (65 536: 1.28 -> 1.01) but the forward pass after it longer by more
    // (1.18 -> 1.52: it starts while the gains are still draining to HBM), so the limit stays at 512.
    const int split_env = tuning().split_bw_tiles;
#define LAUNCH_BW2(F, L)                                                                                       \
    AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,                                              \
        hipLaunchKernelGGL((k_backward2<D, RP, F, L, XT>), dim3(k.ntiles), dim3(2 * TILE), 0, st, k, (const real*)p->ref, \
                           (const XT*)x, u, x0, Kt, lmbd0, status, (const int*)nullptr, (const int*)nullptr)))
#define LAUNCH_BW4(F, L)                                                                                       \
    AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,                                              \
        hipLaunchKernelGGL((k_backward4<D, RP, F, L, XT>), dim3(k.ntiles), dim3(4 * TILE), 0, st, k, (const real*)p->ref, \
                           (const XT*)x, u, x0, Kt, lmbd0, status)))
    // Gauss-Newton iterations of tiny batches (no costate): four wavefronts per tile, see k_backward4.  (With the costate
    // the one producer is the longest chain of the four and the two-wavefront kernel is as fast: 0.55 vs 0.63 ms measured.)
    if (!lam && k.ntiles <= tuning().bw4_tiles && k.ntiles <= split_env && p->T >= 3) {
        if (tuning().bw5) {   // the producer on two wavefronts, see k_backward5
            AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,
                hipLaunchKernelGGL((k_backward5<D, RP, XT>), dim3(k.ntiles), dim3(5 * TILE), 0, st, k, (const real*)p->ref,
                                   (const XT*)x, u, x0, Kt, status)));
        } else {
            LAUNCH_BW4(false, false);
        }
    } else if (k.ntiles <= split_env && p->T >= 3) {
        if (full_hessian) LAUNCH_BW2(true, true);
        else if (lam) LAUNCH_BW2(false, true);
        else LAUNCH_BW2(false, false);
    } else if (full_hessian) LAUNCH_BW(true, true);
    else if (lam) LAUNCH_BW(false, true);
    else LAUNCH_BW(false, false);
#undef LAUNCH_BW4
#undef LAUNCH_BW2
#undef LAUNCH_BW
    return check_launch("k_backward");
}

static int api_gradient(const aoc_problem* p, const void* x, const real* u, const real* x0, real* du, real* slope,
                        int32_t* status) {
    int rc = check_problem(p);
    if (rc) return rc;
    if (!x || !u || !x0 || !du || !slope) return einval("aoc_gradient: NULL argument");
    KConst k = make_const(p);
    AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,
        hipLaunchKernelGGL((k_gradient<D, RP, XT>), dim3(k.ntiles), dim3(TILE), 0, (hipStream_t)p->stream, k, (const real*)p->ref,
                           (const XT*)x, u, x0, du, slope, status)));
    return check_launch("k_gradient");
}

static int api_forward(const aoc_problem* p, const aoc_params* prm, int32_t n_spec, const void* x, const real* u,
                const real* x0, const real* Kt, real* du, real* descent, real* J_trial, int32_t* status,
                void* cand = nullptr, size_t cand_size = 0, const int32_t* ntrials_hint = nullptr) {
    int rc = check_problem(p);
    if (rc) return rc;
    if (!prm || !x || !u || !x0 || !Kt || !du || !descent || !J_trial) return AOC_EINVAL;
    if (n_spec < 1 || n_spec > AOC_SPEC_MAX) return AOC_EINVAL;
    if (cand && cand_size < cand_bytes(p->B, p->T, n_spec))
        return einval("aoc_forward: candidate store of %zu bytes, %zu needed (aoc_candidate_bytes)", cand_size,
                      cand_bytes(p->B, p->T, n_spec));
    KConst k = make_const(p);
    hipStream_t st = (hipStream_t)p->stream;
#define LAUNCH_FW_(N, XR, XT)                                                                                       \
    hipLaunchKernelGGL((k_forward<D, RP, N, XR, XT>), dim3(k.ntiles), dim3(TILE), 0, st, k, *prm, (const real*)p->ref, \
                       (const XT*)x, u, x0, Kt, du, descent, J_trial, status)
#define LAUNCH_FW(N)                                                                                                \
    AOC_DISPATCH_DR(k, D, RP, do {                                                                                  \
        if (!p->x_in_f32) LAUNCH_FW_(N, false, real);                                                               \
        else if (xrc) LAUNCH_FW_(N, true, float);                                                                   \
        else LAUNCH_FW_(N, false, float);                                                                           \
    } while (0))
    // the role kernels of small batches (k_forward_split, _lin, _duo) take the same arguments: GROUPS workgroups per tile of
    // NWAVES wavefronts
#define LAUNCH_FW_ROLES(KERNEL, GROUPS, NWAVES)                                                                      \
    hipLaunchKernelGGL(KERNEL, dim3(k.ntiles, GROUPS), dim3((NWAVES) * TILE), 0, st, k, *prm, n_spec, cb,           \
                       (const real*)p->ref, (const XT*)x, u, x0, Kt, du, descent, J_trial, status, ntrials_hint)
    // the states are re-computed instead of read when the caller says they are the rollout of u (float32 storage only)
    const bool xrc = p->x_is_rollout && p->x_in_f32 && tuning().fw_recompute != 0;
    // small batches: one wavefront per chain, see k_forward_split
    const int split_env = tuning().split_tiles;
    // measured (forward pass, ms): 24 576 trajectories 0.91 -> 0.56, 32 768 (512 tiles) 0.94 -> 0.62, 40 960 0.94 -> 1.07
    const int split_fw = split_env;
    if (n_spec > 3 || (k.ntiles <= split_fw && p->T >= 3)) {   // more than 3 trials: only this kernel takes them
        if (p->T < 3) return AOC_EINVAL;
        const CandBuf cb = cand_carve(cand, p->B, p->T, n_spec);
        // at most one workgroup per CU (256 CUs): the build for one wavefront per SIMD, which keeps the stage in registers
        // (see AOC_FWS_ATTR); aoc_tuning.fw_wpe1 = 0 keeps the two-per-SIMD build for every launch
        const int one_per_cu = tuning().fw_wpe1 ? 256 : 0;
        // nominal-point work on a wavefront of its own (k_forward_lin): measured (tools/small_ab.py, forward pass in ms,
        // k_forward_split -> k_forward_lin): 32 768 trajectories (2 candidates, one workgroup per tile either way) 0.585 -> 0.560;
        // with more candidates its two trials per workgroup need more workgroups per tile than the three of
        // k_forward_split and it loses: 1024 trajectories 0.342 -> 0.364, 4096 0.42 -> 0.48, 8192 0.44 -> 0.79, 16 384 0.44 -> 0.84.
        // The trial wavefronts are the floor of the stage either way (one rollout stage is ~230 instructions at the 5.25-6.6
        // cycles a lone wavefront gets per fp64 instruction), not the LQR wavefront.  aoc_tuning.fw_lin: -1 = where it wins.
        const int fw_lin = tuning().fw_lin;
        // tiny batches whose candidates all ride along: the stage on seven roles, two candidates per workgroup (k_forward_duo)
        const int duo_max = tuning().fw_duo == 1 ? 256 : tuning().fw_duo;   // workgroups the launch may have (1: one per CU)
        if (duo_max > 0 && n_spec > FWS_TPG && k.ntiles * ((n_spec + 1) / 2) <= duo_max) {
            AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT,
                LAUNCH_FW_ROLES((k_forward_duo<D, RP, XT>), (n_spec + FWD_CPG - 1) / FWD_CPG, 8)));
        } else if (fw_lin > 0 || (fw_lin < 0 && n_spec <= FWL_TPG)) {
            const int ngroups = (n_spec + FWL_TPG - 1) / FWL_TPG;
            AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT, AOC_DISPATCH_WPE(k.ntiles * ngroups <= one_per_cu, WPE,
                LAUNCH_FW_ROLES((k_forward_lin<D, RP, XT, WPE>), ngroups, 2 + FWL_TPG))));
        } else {
            const int ngroups = (n_spec + FWS_TPG - 1) / FWS_TPG;
            const int nwaves = 1 + (n_spec < FWS_TPG ? n_spec : FWS_TPG);
            AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_in_f32, XT, AOC_DISPATCH_WPE(k.ntiles * ngroups <= one_per_cu, WPE,
                LAUNCH_FW_ROLES((k_forward_split<D, RP, XT, WPE>), ngroups, nwaves))));
        }
    } else if (n_spec == 1) LAUNCH_FW(1);
    else if (n_spec == 2) LAUNCH_FW(2);
    else LAUNCH_FW(3);
#undef LAUNCH_FW_ROLES
#undef LAUNCH_FW
#undef LAUNCH_FW_
    return check_launch("k_forward");
}

// The line-search scratch: one walk over its layout carves the pointers out of `scratch` (if given) and returns its size
// (aoc_linesearch_scratch_bytes).  (LsState: the fp64 build's in either build, the larger of the two.)
static size_t ls_layout(int ntiles, void* scratch, LsScratch* sc) {
    const size_t nt = (size_t)ntiles;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = scratch ? (char*)scratch + off : nullptr; off += align_up(bytes, 16); return q; };
    LsScratch s;
    s.mask = (unsigned long long*)take(nt * sizeof(unsigned long long));
    s.prefix = (int*)take((nt + 1) * sizeof(int));
    s.first_ok = (int*)take(nt * TILE * sizeof(int));
    s.st = (LsState*)take(sizeof(aoc64::LsState));
    s.items = (int2*)take(nt * TILE * LS_WL_IPL * sizeof(int2));
    s.next_r = (int*)take(nt * TILE * sizeof(int));
    s.wl_count = (int*)take(2 * LS_WL_ROUNDS * sizeof(int));
    if (sc) *sc = s;
    return off;
}

// work-list search (k_ls_init_wl ...) or round-based search (k_ls_init ...): by batch size unless aoc_tuning says otherwise
static bool ls_use_worklist(int ntiles) {
    const aoc_tuning& tn = tuning();
    return tn.ls_worklist > 0 || (tn.ls_worklist < 0 && ntiles > tn.split_tiles);
}

// armijo_stepsize for every trajectory (optcon.py:204-327): see aoc_linesearch_search in include/aoc.h
static int api_ls_search(const aoc_problem* p, const aoc_params* prm, int32_t n_spec, const real* u, const real* x0,
                         const real* du, const real* J_cur, const real* descent, const real* J_trial0, real* stepsize,
                         int32_t* ntrials, void* scratch, size_t scratch_size, LsFrozen frozen = LsFrozen{nullptr, nullptr}) {
    int rc = check_problem(p);
    if (rc) return rc;
    if (!prm || !u || !x0 || !du || !J_cur || !descent || (!J_trial0 && n_spec > 0) || !stepsize || !ntrials || !scratch)
        return einval("aoc_linesearch: NULL argument");
    if (scratch_size < aoc_linesearch_scratch_bytes(p->B, p->T))
        return einval("aoc_linesearch: scratch of %zu bytes, %zu needed (aoc_linesearch_scratch_bytes)", scratch_size,
                      aoc_linesearch_scratch_bytes(p->B, p->T));
    if (prm->armijo_maxiters < 1 || prm->armijo_maxiters >= LS_MAX_STEPS)
        return einval("aoc_linesearch: armijo_maxiters = %d (1 .. %d)", prm->armijo_maxiters, LS_MAX_STEPS - 1);
    if (n_spec < 0 || n_spec > AOC_SPEC_MAX) return einval("aoc_linesearch: n_spec = %d (0 .. %d)", n_spec, AOC_SPEC_MAX);
    KConst k = make_const(p);
    hipStream_t st = (hipStream_t)p->stream;
    LsScratch sc;
    ls_layout(k.ntiles, scratch, &sc);
    const aoc_tuning& tn = tuning();
    if (ls_use_worklist(k.ntiles)) {
        // work-list search: two rounds for armijo_maxiters <= n_spec + LS_WL_IPL * cpl (one more per further
        // LS_WL_IPL * cpl candidates), see k_ls_init_wl
        const int cpl = tn.ls_cpl >= 4 ? 4 : tn.ls_cpl >= 2 ? 2 : 1;
        if (prm->armijo_maxiters > 255) return einval("aoc_linesearch: armijo_maxiters > 255");
        const int remaining = prm->armijo_maxiters > n_spec ? prm->armijo_maxiters - n_spec : 0;
        const int per_round = LS_WL_IPL * cpl;
        const int nrounds = remaining > 0 ? 1 + (remaining + per_round - 1) / per_round : 0;
        if (nrounds > LS_WL_ROUNDS)
            return einval("aoc_linesearch: armijo_maxiters = %d needs more than %d work-list rounds", prm->armijo_maxiters,
                          LS_WL_ROUNDS);
        if (hipMemsetAsync(sc.wl_count, 0, 2 * LS_WL_ROUNDS * sizeof(int), st) != hipSuccess)
            return check_launch("aoc_linesearch");
        hipLaunchKernelGGL(k_ls_init_wl, dim3(k.ntiles), dim3(TILE), 0, st, *prm, n_spec, cpl,
                           tn.ls_depth_min > 1 ? tn.ls_depth_min : 1, k.ntiles * TILE, J_cur, descent, J_trial0, stepsize,
                           ntrials, sc, frozen);
        const int ipl = (remaining + cpl - 1) / cpl < LS_WL_IPL ? (remaining + cpl - 1) / cpl : LS_WL_IPL;
        // every remaining candidate at once while that keeps the first round within about two wavefronts per SIMD
        // (measured, B = 131 072: 1024 -> 2048 wavefronts -0.03 ms per iteration; the kernel runs 7 per SIMD)
        const int wcap = tn.ls_wcap > 0 ? tn.ls_wcap : 2048;
        for (int r = 0; r < nrounds; r++) {
            if (r == 0)
                hipLaunchKernelGGL(k_ls_plan_wl, dim3(k.ntiles), dim3(TILE), 0, st, prm->armijo_maxiters, n_spec, cpl,
                                   wcap * TILE, sc);
            else
                hipLaunchKernelGGL(k_ls_replan, dim3(k.ntiles), dim3(TILE), 0, st, prm->armijo_maxiters, cpl, r, stepsize,
                                   ntrials, sc);
#define LAUNCH_WL(C, PINNED)                                                                                      \
    AOC_DISPATCH_DR(k, D, RP,                                                                                  \
        hipLaunchKernelGGL((k_ls_trial_wl<D, RP, C, PINNED>), dim3(k.ntiles * ipl), dim3(TILE), 0, st, k, *prm, r,    \
                           (const real*)p->ref, u, x0, du, J_cur, descent, sc))
            if (cpl == 4) LAUNCH_WL(4, false);
            else if (cpl == 2) LAUNCH_WL(2, false);
            else {   // the size of the round is known on the device only: one of the two does the work
                LAUNCH_WL(1, true);
                LAUNCH_WL(1, false);
            }
#undef LAUNCH_WL
        }
        return check_launch("aoc_linesearch");
    }
    // wavefronts a trial round may occupy: about one per SIMD (256 CUs x 4 SIMDs), at least one per tile
    const int wcap_env = tn.ls_wcap > 0 ? tn.ls_wcap : 1024;
    // speculation depth of round n is at most kgrow*n + 1: small batches leave most SIMDs idle, so their first
    // round may as well try every remaining step (measured: B <= 16 384 -13..15 % per iteration with kgrow = 9,
    // B = 131 072 +8 % on the line search)
    const int kgrow_set = tn.ls_kgrow;
    const int kgrow_env = kgrow_set > 0 ? kgrow_set : (k.ntiles <= 512 ? 9 : 1);
    const int wcap = k.ntiles > wcap_env ? k.ntiles : wcap_env;
    const bool trial_split = tn.trial_split != 0 && p->T >= 3;
    hipLaunchKernelGGL(k_ls_init, dim3(k.ntiles), dim3(TILE), 0, st, *prm, n_spec, k.ntiles * TILE, J_cur, descent,
                       J_trial0, stepsize, ntrials, sc, frozen);
    // At most LS_ROUNDS rounds: the depth K grows per round (2, 3, 4, ...) and the last launched round takes
    // every remaining step index, so that ~3 rounds cover armijo_maxiters = 10 and the launches of rounds
    // that turn out empty stay few.
    const int remaining = prm->armijo_maxiters - n_spec;
    int nrounds = remaining < LS_ROUNDS ? remaining : LS_ROUNDS;
    // small batches: the first round is known to take every remaining step of every searching trajectory
    // (k_ls_plan: K = min(wcap / nw, kgrow + 1) >= remaining), the later rounds would be empty launches
    if (nrounds > 1 && (long)k.ntiles * remaining <= wcap_env && kgrow_env + 1 >= remaining) nrounds = 1;
    for (int r = 0; r < nrounds; r++) {
        const int last = (r == nrounds - 1);
        if (r > 0) hipLaunchKernelGGL(k_ls_resolve, dim3(k.ntiles), dim3(TILE), 0, st, sc, stepsize, ntrials);
        hipLaunchKernelGGL(k_ls_plan, dim3(1), dim3(1024), 0, st, k.ntiles, prm->armijo_maxiters, wcap_env, kgrow_env,
                           last, sc);
        const int grid = last ? k.ntiles * (remaining > 1 ? remaining : 1) : wcap;  // K * nw <= grid
        if (trial_split && k.ntiles <= 512) {
            AOC_DISPATCH_DR(k, D, RP,
                hipLaunchKernelGGL((k_ls_trial_split<D, RP>), dim3(grid), dim3(2 * TILE), 0, st, k, *prm, (const real*)p->ref, u,
                                   x0, du, J_cur, descent, sc));
        } else {
            AOC_DISPATCH_DR(k, D, RP,
                hipLaunchKernelGGL((k_ls_trial<D, RP>), dim3(grid), dim3(TILE), 0, st, k, *prm, (const real*)p->ref, u, x0, du,
                                   J_cur, descent, sc));
        }
    }
    return check_launch("aoc_linesearch");
}

// get_update with the step the search found (optcon.py:488-491): see aoc_linesearch_update in include/aoc.h
static int api_ls_update(const aoc_problem* p, const aoc_params* prm, const real* u, const real* x0, const real* du,
                         void* x_new, real* u_new, real* J_new, real* stepsize, int32_t* ntrials, int32_t* status,
                         void* scratch, size_t scratch_size, int32_t n_spec = 0, const real* J_trial = nullptr,
                         const void* cand = nullptr, size_t cand_size = 0) {
    int rc = check_problem(p);
    if (rc) return rc;
    if (!prm || !u || !x0 || !du || !x_new || !u_new || !J_new || !stepsize || !ntrials || !scratch)
        return einval("aoc_linesearch: NULL argument");
    if (scratch_size < aoc_linesearch_scratch_bytes(p->B, p->T))
        return einval("aoc_linesearch: scratch of %zu bytes, %zu needed (aoc_linesearch_scratch_bytes)", scratch_size,
                      aoc_linesearch_scratch_bytes(p->B, p->T));
    if (cand && J_trial && (n_spec < 1 || n_spec > AOC_SPEC_MAX || cand_size < cand_bytes(p->B, p->T, n_spec)))
        return einval("aoc_linesearch: candidate store of %zu bytes for n_spec = %d, %zu needed (aoc_candidate_bytes)", cand_size,
                      n_spec, n_spec >= 1 && n_spec <= AOC_SPEC_MAX ? cand_bytes(p->B, p->T, n_spec) : (size_t)0);
    if (prm->armijo_maxiters < 1 || prm->armijo_maxiters >= LS_MAX_STEPS)
        return einval("aoc_linesearch: armijo_maxiters = %d (1 .. %d)", prm->armijo_maxiters, LS_MAX_STEPS - 1);
    KConst k = make_const(p);
    hipStream_t st = (hipStream_t)p->stream;
    LsScratch sc;
    ls_layout(k.ntiles, scratch, &sc);
    if (k.ntiles <= tuning().split_tiles && p->T >= 3) {   // small batches: state chain and cost on two wavefronts
        // candidates the forward pass stored (aoc_forward with `cand`): the update of most tiles is then a copy
        const CandBuf cb = cand_carve(J_trial ? cand : nullptr, p->B, p->T, n_spec);
        AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_out_f32, XO,
            hipLaunchKernelGGL((k_ls_final_split<D, RP, XO>), dim3(k.ntiles, cb.n > 0 ? LSF_NY : 1), dim3(2 * TILE), 0, st, k,
                               prm->armijo_maxiters, cb, J_trial, (const real*)p->ref, u, x0, du, (XO*)x_new, u_new, J_new,
                               stepsize, ntrials, status, sc)));
    } else {
        AOC_DISPATCH_DR(k, D, RP, AOC_DISPATCH_XT(p->x_out_f32, XO,
            hipLaunchKernelGGL((k_ls_final<D, RP, XO>), dim3(k.ntiles), dim3(TILE), 0, st, k, prm->armijo_maxiters,
                               (const real*)p->ref, u, x0, du, (XO*)x_new, u_new, J_new, stepsize, ntrials, status, sc)));
    }
    return check_launch("aoc_linesearch");
}

static int api_linesearch(const aoc_problem* p, const aoc_params* prm, int32_t n_spec, const real* u, const real* x0,
                   const real* du, const real* J_cur, const real* descent, const real* J_trial0,
                   void* x_new, real* u_new, real* J_new, real* stepsize, int32_t* ntrials, int32_t* status,
                   void* scratch, size_t scratch_size, LsFrozen frozen = LsFrozen{nullptr, nullptr}, const void* cand = nullptr,
                   size_t cand_size = 0) {
    if (!x_new || !u_new || !J_new) return einval("aoc_linesearch: NULL argument");
    const int rc = api_ls_search(p, prm, n_spec, u, x0, du, J_cur, descent, J_trial0, stepsize, ntrials, scratch, scratch_size, frozen);
    if (rc) return rc;
    return api_ls_update(p, prm, u, x0, du, x_new, u_new, J_new, stepsize, ntrials, status, scratch, scratch_size, n_spec,
                         J_trial0, cand, cand_size);
}

static int api_lqr_tracking(const aoc_problem* p, const void* x_opt, const real* u_opt, const real* x_opt0,
                     const real* x0_reg, real* Kgain, void* x_reg, real* u_reg, int32_t* status,
                     void* scratch = nullptr, size_t scratch_bytes = 0) {
    int rc = check_problem(p);
    if (!rc) rc = check_riccati_weights(p, "aoc_lqr_tracking");
    if (rc) return rc;
    if (!x_opt || !u_opt || !x_opt0 || !Kgain) return AOC_EINVAL;
    if ((x_reg == nullptr) != (u_reg == nullptr) || (x_reg && !x0_reg)) return AOC_EINVAL;
    KConst k = make_const(p);
    hipStream_t st = (hipStream_t)p->stream;
    const int split_tiles = tuning().split_tiles;
    const HcutPlan pl = hcut_plan(HCUT_TRACK, tuning().track_hcut, k.ntiles, k.ntiles, p->T, scratch, scratch_bytes);
    if (pl.cut) {
        // the horizon in S segments (see k_track_hcut_map): for batches that leave most SIMDs idle
        const int S = pl.S;
        if (pl.multiwave) {   // every wavefront of the segment kernels still on a SIMD of its own
            AOC_DISPATCH_BOOL(k.diag, D, AOC_DISPATCH_XT(p->x_in_f32, XT,
                hipLaunchKernelGGL((k_track_hcut_map3<D, XT>), dim3(k.ntiles, S), dim3(3 * TILE), 0, st, k, S, (const XT*)x_opt, u_opt,
                                   x_opt0, Kgain, (real*)scratch, status)));
        } else {
            AOC_DISPATCH_BOOL(k.diag, D, AOC_DISPATCH_XT(p->x_in_f32, XT,
                hipLaunchKernelGGL((k_track_hcut_map<D, XT>), dim3(k.ntiles, S), dim3(TILE), 0, st, k, S, (const XT*)x_opt, u_opt,
                                   x_opt0, Kgain, (real*)scratch, status)));
        }
        hcut_launch_chain<false>(k.ntiles, S, (real*)scratch, st);
        if (pl.multiwave) {
            AOC_DISPATCH_BOOL(k.diag, D, AOC_DISPATCH_XT(p->x_in_f32, XT,
                hipLaunchKernelGGL((k_track_hcut_gains2<D, XT>), dim3(k.ntiles, S - 1), dim3(2 * TILE), 0, st, k, S, (const XT*)x_opt, u_opt,
                                   x_opt0, Kgain, (const real*)scratch, status)));
        } else {
            AOC_DISPATCH_BOOL(k.diag, D, AOC_DISPATCH_XT(p->x_in_f32, XT,
                hipLaunchKernelGGL((k_track_hcut_gains<D, XT>), dim3(k.ntiles, S - 1), dim3(TILE), 0, st, k, S, (const XT*)x_opt, u_opt,
                                   x_opt0, Kgain, (const real*)scratch, status)));
        }
    } else if (k.ntiles <= split_tiles && k.ntiles <= tuning().bw4_tiles && p->T >= 3) {
        AOC_DISPATCH_BOOL(k.diag, D, AOC_DISPATCH_XT(p->x_in_f32, XT,
            hipLaunchKernelGGL((k_track_gains4<D, XT>), dim3(k.ntiles), dim3(4 * TILE), 0, st, k, (const XT*)x_opt, u_opt,
                               x_opt0, Kgain, status)));
    } else if (k.ntiles <= split_tiles && p->T >= 3) {
        AOC_DISPATCH_BOOL(k.diag, D, AOC_DISPATCH_XT(p->x_in_f32, XT,
            hipLaunchKernelGGL((k_track_gains2<D, XT>), dim3(k.ntiles), dim3(2 * TILE), 0, st, k, (const XT*)x_opt, u_opt,
                               x_opt0, Kgain, status)));
    } else {
        AOC_DISPATCH_BOOL(k.diag, D, AOC_DISPATCH_XT(p->x_in_f32, XT,
            hipLaunchKernelGGL((k_track_gains<D, XT>), dim3(k.ntiles), dim3(TILE), 0, st, k, (const XT*)x_opt, u_opt, x_opt0,
                               Kgain, status)));
    }
    if (x_reg)
        AOC_DISPATCH_XT(p->x_in_f32, XT, AOC_DISPATCH_XT(p->x_out_f32, XO,
            hipLaunchKernelGGL((k_track_rollout<XT, XO>), dim3(k.ntiles), dim3(TILE), 0, st, k, (const XT*)x_opt, u_opt,
                               x_opt0, Kgain, x0_reg, (XO*)x_reg, u_reg, status)));
    return check_launch("aoc_lqr_tracking");
}

static int api_ltv_lqr(int32_t nb, int32_t T, int32_t augmented, const real* A, const real* Bm, const real* Q,
                const real* R, const real* S, const real* Qf, const real* x0, const real* q,
                const real* r, const real* qf, real* KK, real* PP, real* xx, real* uu, int32_t* nreg,
                int32_t* nsing, void* stream) {
    if (nb < 1 || T < 2 || !A || !Bm || !Q || !R || !S || !Qf || !x0 || !KK || !PP || !xx || !uu) return AOC_EINVAL;
    if (!augmented && (q || r || qf)) return AOC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((nb + 63) / 64), blk(64);
    if (augmented)
        hipLaunchKernelGGL(k_ltv_lqr<7>, grid, blk, 0, st, nb, T, A, Bm, Q, R, S, Qf, x0, q, r, qf, KK, PP, xx, uu, nreg, nsing);
    else
        hipLaunchKernelGGL(k_ltv_lqr<6>, grid, blk, 0, st, nb, T, A, Bm, Q, R, S, Qf, x0, q, r, qf, KK, PP, xx, uu, nreg, nsing);
    return check_launch("k_ltv_lqr");
}

// Candidates aoc_newton_iterate lets the forward pass store (CandBuf): only where ALL candidates ride along in the
// forward pass (a tile is then updated by copying unless a search was exhausted) and the forward pass has at most one
// workgroup per CU — measured: 4096 trajectories forward +0.07 ms for the stores, update -0.21 ms; 8192 trajectories
// (two workgroups per CU) +0.22 / -0.19 ms; with fewer candidates than armijo_maxiters hardly any tile qualifies.
// The workspace is sized for the largest count the batch size allows, whatever armijo_maxiters turns out to be.
static int cand_count(int32_t B, int32_t n_spec, int32_t armijo_maxiters) {
    const int groups = (n_spec + FWS_TPG - 1) / FWS_TPG;
    return n_spec > FWS_TPG && n_spec >= armijo_maxiters && aoc_ntiles(B) * groups <= 256 ? n_spec : 0;
}

// what one iteration needs in any case: K~ (14) + du (2) components, tiled; trial costs; the line-search scratch
static size_t ws_base_bytes(int32_t B, int32_t T) {
    return aoc_tiled_elems(B, T, 16) * sizeof(real) + AOC_SPEC_MAX * (size_t)aoc_ntiles(B) * TILE * sizeof(real) +
           align_up(aoc_linesearch_scratch_bytes(B, T), 256);
}

// Largest number of stored (tile, candidate) pairs a batch of at most `ntiles` tiles can have: a batch stores n =
// armijo_maxiters candidates only if all of them ride along (n > FWS_TPG) on at most 256 workgroups of FWS_TPG
// candidates, tiles x ceil(n / FWS_TPG) <= 256 (cand_count).  exact = only the batch of exactly `ntiles` tiles.
static size_t cand_pairs_max(int ntiles, bool exact) {
    size_t best = 0;
    for (int n = FWS_TPG + 1; n <= AOC_SPEC_MAX; n++) {
        const int groups = (n + FWS_TPG - 1) / FWS_TPG;
        int t = 256 / groups;
        if (exact) { if (ntiles > t) continue; t = ntiles; }
        else if (t > ntiles) t = ntiles;
        if ((size_t)n * t > best) best = (size_t)n * t;
    }
    return best;
}
// bytes of `pairs` stored (tile, candidate) trajectories + the per-tile counts, as cand_bytes() lays them out
static size_t cand_region_bytes(size_t pairs, int32_t T, int ntiles) {
    return pairs ? pairs * ((size_t)T * TILE * CAND_REC_BYTES + (size_t)TILE * sizeof(int)) + align_up((size_t)ntiles * sizeof(int), 16) : 0;
}

// aoc_workspace_bytes: what a batch of exactly B trajectories needs — K~ (14) + du (2) components, tiled; trial costs
// [AOC_SPEC_MAX][ntiles*64]; the line-search scratch; the candidate store if a batch of this size keeps one (whatever
// armijo_maxiters turns out to be).
static size_t api_workspace_bytes(int32_t B, int32_t T) {
    const int nt = aoc_ntiles(B);
    return ws_base_bytes(B, T) + cand_region_bytes(cand_pairs_max(nt, true), T, nt);
}
// ... and what serves every batch of AT MOST B trajectories: aoc_newton_solve runs its re-packed, smaller generations in
// the workspace of the first, and a smaller batch may store candidates where B does not.
static size_t api_workspace_bytes_upto(int32_t B, int32_t T) {
    const int nt = aoc_ntiles(B);
    return ws_base_bytes(B, T) + cand_region_bytes(cand_pairs_max(nt, false), T, nt < 256 ? nt : 256);
}

static int api_newton_iterate(const aoc_problem* p, const aoc_params* prm, int32_t kk, const void* x, const real* u,
                       const real* x0, const real* J_cur, void* workspace, size_t workspace_bytes, void* x_new, real* u_new,
                       real* J_new, real* descent, real* stepsize, int32_t* ntrials, int32_t* status,
                       LsFrozen frozen = LsFrozen{nullptr, nullptr}, int hcut_ntiles = 0) {
    int rc = check_problem(p);
    if (!rc) rc = check_riccati_weights(p, sizeof(real) == 8 ? "aoc_newton_iterate" : "aoc_newton_iterate_f32");
    if (rc) return rc;
    if (!prm || !workspace) return einval("aoc_newton_iterate: NULL argument");
    if (workspace_bytes < ws_base_bytes(p->B, p->T))
        return einval("aoc_newton_iterate: workspace of %zu bytes, %zu needed (aoc_workspace_bytes)", workspace_bytes,
                      ws_base_bytes(p->B, p->T));
    real* Kt = (real*)workspace;
    real* du = Kt + aoc_tiled_elems(p->B, p->T, 14);
    real* J_trial = du + aoc_tiled_elems(p->B, p->T, 2);
    char* scratch = (char*)(J_trial + AOC_SPEC_MAX * (size_t)aoc_ntiles(p->B) * TILE);
    const int nspec = aoc_default_nspec(p->B, prm->armijo_maxiters);
    // the candidate store is used only if the workspace handed over has room for it
    const int ncand = tuning().store_candidates ? cand_count(p->B, nspec, prm->armijo_maxiters) : 0;
    void* cand = ncand && ws_base_bytes(p->B, p->T) + cand_bytes(p->B, p->T, ncand) <= workspace_bytes
                     ? scratch + align_up(aoc_linesearch_scratch_bytes(p->B, p->T), 256) : nullptr;
    // everything behind K~ in the workspace (du, trial costs, line-search scratch, candidate store) is written only by the
    // passes that follow: the backward pass may use it as scratch
    rc = api_backward(p, kk > prm->hessian_switch, x, u, x0, Kt, nullptr, status, du,
                      workspace_bytes - aoc_tiled_elems(p->B, p->T, 14) * sizeof(real), hcut_ntiles);
    if (rc) return rc;
    // `ntrials` still holds the trial counts of the previous iteration (zeros before the first): how deep to store
    const size_t cand_size = cand ? cand_bytes(p->B, p->T, ncand) : 0;
    rc = api_forward(p, prm, nspec, x, u, x0, Kt, du, descent, J_trial, status, cand, cand_size, ntrials);
    if (rc) return rc;
    return api_linesearch(p, prm, nspec, u, x0, du, J_cur, descent, J_trial, x_new, u_new, J_new, stepsize, ntrials,
                          status, scratch, aoc_linesearch_scratch_bytes(p->B, p->T), frozen, cand, cand_size);
}


