// passes/lqg.inc — tracking ensembles with noisy measurements and a Kalman estimate in the loop (aoc_track_ensemble_lqg), and
// the same loop with actuator limits (aoc_track_ensemble_lqg_limited).
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// No kernel of its own: the F_t / c_t records are those of k_cov_stage (covariance.inc), launched as it is into the call's
// scratch, and the loop is the EST instance of k_track_ensemble (ensemble.inc), which reads them.  The estimator is
// instantiated for the trajectories and the statistics-only forms alone, not together with the envelope or the histogram.
// With limits the loop is the EST && LIM instance, the records are those of k_cov_stage<true, true> — the entries of B_t
// where the copy of K lay, which this loop never reads — and the tiles' cut counts are folded by k_sat_fold as they are
// for aoc_track_ensemble_limited.
// ---------------------------------------------------------------------------------------------
#ifndef AOC_KERNELS_ONLY
static_assert(EST_FC == COV_REC && EST_O_C == COV_O_C, "the estimator instances read the records k_cov_stage writes");
static_assert(EST_O_B == COV_O_K && EST_O_B % 2 == 0, "b20, b50 lie where the record's copy of K starts, on 16 bytes");

// aoc_track_ensemble_lqg_scratch_bytes: the records of k_cov_stage, [n_opt][T][COV_REC]; 0 for a geometry the call refuses anyway
static size_t track_ensemble_lqg_scratch_bytes(int32_t n_opt, int32_t T) { return track_covariance_scratch_bytes(n_opt, T); }

// aoc_track_ensemble_lqg_limited_scratch_bytes: those records, rounded up to 16 bytes, then the cut counts' cnt[ntiles][T][2]
// int32 if sat_count is asked for; 0 for a geometry the call refuses anyway
static size_t track_ensemble_lqg_limited_scratch_bytes(int32_t B, int32_t n_opt, int32_t T, int32_t members_per_opt,
                                                       int32_t with_sat_count) {
    if (B < 1 || n_opt < 1 || T < 3 || members_per_opt < TILE || members_per_opt % TILE) return 0;
    if ((long long)B <= (long long)(n_opt - 1) * members_per_opt || (long long)B > (long long)n_opt * members_per_opt) return 0;
    const size_t own = track_ensemble_lqg_scratch_bytes(n_opt, T);
    return ((own + 15) & ~(size_t)15) + (with_sat_count ? (size_t)((B + TILE - 1) / TILE) * (size_t)T * 2 * sizeof(int) : 0);
}

// Body of aoc_track_ensemble_lqg and, `limited` with limits, est_input, sat (not NULL) and sat_count (may be NULL), of
// aoc_track_ensemble_lqg_limited; fn the name of the entry point for the reasons.  A template only so that the kernels it
// names are instantiated where it is called — from the fp64 entry points — and not once more in the float32 namespace.
template <typename = void>
static int api_track_ensemble_lqg(const char* fn, const aoc_problem* p, int32_t n_opt, int32_t members_per_opt,
                                  const real* nominal, const real* filter, const real* x0_reg, const real* ehat0,
                                  const aoc_mpc_noise* noise, const double* rho, void* x_reg, real* u_reg, real* xhat_reg,
                                  real* dist_out, real* meas_out, real* stats, real* est_stats, int32_t* status, void* scratch,
                                  size_t scratch_bytes, bool limited = false, const aoc_actuator_limits* limits = nullptr,
                                  int32_t est_input = 0, real* sat = nullptr, int32_t* sat_count = nullptr) {
    const char* missing = !filter ? "filter" : (!est_stats ? "est_stats" : nullptr);
    if (int rc = ens_check_args(fn, p, n_opt, members_per_opt, nominal, x0_reg, noise, x_reg, u_reg, stats, missing)) return rc;
    bool draws = false;
    if (rho) {
        if (!noise) return einval("%s: rho without noise (the seed of the measurement draws is noise->seed; its sigma may be 0)", fn);
        for (int c = 0; c < 6; c++) {
            if (!(rho[c] >= 0.0) || !__builtin_isfinite(rho[c]))
                return einval("%s: rho[%d] = %g (need a finite rho >= 0)", fn, c, rho[c]);
            draws = draws || rho[c] > 0.0;
        }
    }
    const char* query = limited ? "aoc_track_ensemble_lqg_limited_scratch_bytes" : "aoc_track_ensemble_lqg_scratch_bytes";
    const size_t need = limited ? track_ensemble_lqg_limited_scratch_bytes(p->B, n_opt, p->T, members_per_opt, sat_count != nullptr)
                                : track_ensemble_lqg_scratch_bytes(n_opt, p->T);
    if (!scratch) return einval("%s: scratch is NULL (need %zu bytes, %s)", fn, need, query);
    if ((uintptr_t)scratch % 16) return einval("%s: scratch must be 16-byte aligned", fn);
    if (scratch_bytes < need) return einval("%s: scratch_bytes = %zu, need %zu (%s)", fn, scratch_bytes, need, query);
    if (limited) {
        if (!limits) return einval("%s: limits is NULL", fn);
        if (!sat) return einval("%s: sat is NULL", fn);
        for (int r = 0; r < 2; r++) {
            if (limits->lo[r] != limits->lo[r] || limits->hi[r] != limits->hi[r] || limits->rate[r] != limits->rate[r])
                return einval("%s: limits has a NaN in channel %d (lo = %g, hi = %g, rate = %g; infinite values mean none)", fn, r,
                              limits->lo[r], limits->hi[r], limits->rate[r]);
            if (limits->lo[r] > limits->hi[r])
                return einval("%s: limits.lo[%d] = %g > limits.hi[%d] = %g", fn, r, limits->lo[r], r, limits->hi[r]);
            if (limits->rate[r] <= 0)
                return einval("%s: limits.rate[%d] = %g (need rate > 0; +inf means none)", fn, r, limits->rate[r]);
        }
        if (est_input != AOC_EST_INPUT_DEMANDED && est_input != AOC_EST_INPUT_APPLIED)
            return einval("%s: est_input = %d (0 the demand, 1 the applied input)", fn, est_input);
    }
    hipStream_t st = (hipStream_t)p->stream;
    // F_t, c_t of every (optimum, sample): the first kernel of aoc_track_covariance, as it is (limited: with b20, b50 in it)
    const KConst kn = make_const(p->model, nullptr, nullptr, nullptr, n_opt, p->T);
    const size_t total = (size_t)n_opt * p->T;
    const dim3 cgrid((unsigned)((total + COV_THREADS - 1) / COV_THREADS));
    if (limited)
        hipLaunchKernelGGL((k_cov_stage<true, true>), cgrid, dim3(COV_THREADS), 0, st, kn, n_opt, nominal, (real*)scratch);
    else
        hipLaunchKernelGGL(k_cov_stage<>, cgrid, dim3(COV_THREADS), 0, st, kn, n_opt, nominal, (real*)scratch);
    if (int rc = check_launch(fn)) return rc;
    KConst k = make_const(p->model, p->QQt, p->RRt, p->QQT, p->B, p->T);
    const MpcNoise nz = ens_noise(noise);
    EnsEst<true> est;
    est.fc = (const real*)scratch;
    est.filter = filter;
    est.ehat0 = ehat0;
    est.mz = nz;   // the disturbance's key, step and first; sigma = rho
    for (int c = 0; c < 6; c++) est.mz.sigma[c] = rho ? rho[c] : 0.0;
    est.mz.on = draws ? 1 : 0;
    est.xhat_reg = xhat_reg;
    est.meas_out = meas_out;
    est.est_stats = est_stats;
    const int tpo = members_per_opt / TILE;
    const bool write = x_reg || dist_out || xhat_reg || meas_out;
    EnsLim<true> lm;
    EnsEstLim<true> el;
    int* cnt = nullptr;
    if (limited) {
        for (int r = 0; r < 2; r++) {
            lm.lo[r] = limits->lo[r];
            lm.hi[r] = limits->hi[r];
            lm.s[r] = limits->rate[r] * p->model.dt;   // the slew per sample, formed once, here
        }
        if (sat_count) cnt = (int*)((char*)scratch + track_ensemble_lqg_limited_scratch_bytes(p->B, n_opt, p->T, members_per_opt, 0));
        lm.sat = sat;
        lm.cnt = cnt;
        el.applied = est_input == AOC_EST_INPUT_APPLIED ? 1 : 0;
    }
#define AOC_LQG_LAUNCH(W, N, XO, D)                                                                                        \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D, false, false, true>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo,     \
                       nominal, x0_reg, nz, (XO*)x_reg, u_reg, dist_out, stats, status, (real*)nullptr, (const real*)nullptr, est)
#define AOC_LQG_LIM_LAUNCH(W, N, XO, D)                                                                                    \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D, false, false, true, true>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo, \
                       nominal, x0_reg, nz, (XO*)x_reg, u_reg, dist_out, stats, status, (real*)nullptr, (const real*)nullptr, est, \
                       lm, el)
#define AOC_LQG_DISPATCH(LAUNCH)                                                                                           \
    do {                                                                                                                   \
        if (p->x_out_f32 && x_reg) /* (never with noise, see ens_check_args) */                                            \
            AOC_DISPATCH_BOOL(k.diag, D, LAUNCH(true, false, float, D));                                                   \
        else                                                                                                               \
            AOC_DISPATCH_BOOL(write, W, AOC_DISPATCH_BOOL(nz.on, N, AOC_DISPATCH_BOOL(k.diag, D, LAUNCH(W, N, double, D)))); \
    } while (0)
    if (limited)
        AOC_LQG_DISPATCH(AOC_LQG_LIM_LAUNCH);
    else
        AOC_LQG_DISPATCH(AOC_LQG_LAUNCH);
#undef AOC_LQG_DISPATCH
#undef AOC_LQG_LIM_LAUNCH
#undef AOC_LQG_LAUNCH
    if (int rc = check_launch(fn)) return rc;
    if (!cnt) return AOC_OK;
    // the cut counts of the tiles folded into sat_count
    const size_t nsat = (size_t)n_opt * p->T * 2;
    hipLaunchKernelGGL(k_sat_fold<>, dim3((unsigned)((nsat + ENV_FOLD_THREADS - 1) / ENV_FOLD_THREADS)), dim3(ENV_FOLD_THREADS),
                       0, st, n_opt, p->T, k.ntiles, tpo, (const int*)cnt, sat_count);
    return check_launch(fn);
}
#endif  // AOC_KERNELS_ONLY
