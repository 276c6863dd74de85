// passes/lqg.inc — tracking ensembles with noisy measurements and a Kalman estimate in the loop (aoc_track_ensemble_lqg).
// Part of aoc_passes.inc (included inside namespace AOC_ARITH_NS, once per arithmetic type); not a translation unit of its own.
// ---------------------------------------------------------------------------------------------
// No kernel of its own: the F_t / c_t records are those of k_cov_stage (covariance.inc), launched as it is into the call's
// scratch, and the loop is the EST instance of k_track_ensemble (ensemble.inc), which reads them.  The estimator is
// instantiated for the trajectories and the statistics-only forms alone, not together with the envelope or the histogram.
// ---------------------------------------------------------------------------------------------
#ifndef AOC_KERNELS_ONLY
static_assert(EST_FC == COV_REC && EST_O_C == COV_O_C, "the estimator instances read the records k_cov_stage writes");

// aoc_track_ensemble_lqg_scratch_bytes: the records of k_cov_stage, [n_opt][T][COV_REC]; 0 for a geometry the call refuses anyway
static size_t track_ensemble_lqg_scratch_bytes(int32_t n_opt, int32_t T) { return track_covariance_scratch_bytes(n_opt, T); }

// Body of aoc_track_ensemble_lqg.  A template only so that the kernels it names are instantiated where it is called — from
// the fp64 entry point — and not once more in the float32 namespace.
template <typename = void>
static int api_track_ensemble_lqg(const aoc_problem* p, int32_t n_opt, int32_t members_per_opt, const real* nominal,
                                  const real* filter, const real* x0_reg, const real* ehat0, const aoc_mpc_noise* noise,
                                  const double* rho, void* x_reg, real* u_reg, real* xhat_reg, real* dist_out, real* meas_out,
                                  real* stats, real* est_stats, int32_t* status, void* scratch, size_t scratch_bytes) {
    const char* fn = "aoc_track_ensemble_lqg";
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
    const size_t need = track_ensemble_lqg_scratch_bytes(n_opt, p->T);
    if (!scratch) return einval("%s: scratch is NULL (need %zu bytes, aoc_track_ensemble_lqg_scratch_bytes)", fn, need);
    if ((uintptr_t)scratch % 16) return einval("%s: scratch must be 16-byte aligned", fn);
    if (scratch_bytes < need)
        return einval("%s: scratch_bytes = %zu, need %zu (aoc_track_ensemble_lqg_scratch_bytes)", fn, scratch_bytes, need);
    hipStream_t st = (hipStream_t)p->stream;
    // F_t, c_t of every (optimum, sample): the first kernel of aoc_track_covariance, as it is
    const KConst kn = make_const(p->model, nullptr, nullptr, nullptr, n_opt, p->T);
    const size_t total = (size_t)n_opt * p->T;
    hipLaunchKernelGGL(k_cov_stage<>, dim3((unsigned)((total + COV_THREADS - 1) / COV_THREADS)), dim3(COV_THREADS), 0, st, kn,
                       n_opt, nominal, (real*)scratch);
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
#define AOC_LQG_LAUNCH(W, N, XO, D)                                                                                        \
    hipLaunchKernelGGL((k_track_ensemble<W, N, XO, D, false, false, true>), dim3(k.ntiles), dim3(TILE), 0, st, k, tpo,     \
                       nominal, x0_reg, nz, (XO*)x_reg, u_reg, dist_out, stats, status, (real*)nullptr, (const real*)nullptr, est)
    if (p->x_out_f32 && x_reg)   // (never with noise, see ens_check_args)
        AOC_DISPATCH_BOOL(k.diag, D, AOC_LQG_LAUNCH(true, false, float, D));
    else
        AOC_DISPATCH_BOOL(write, W, AOC_DISPATCH_BOOL(nz.on, N, AOC_DISPATCH_BOOL(k.diag, D, AOC_LQG_LAUNCH(W, N, double, D))));
#undef AOC_LQG_LAUNCH
    return check_launch(fn);
}
#endif  // AOC_KERNELS_ONLY
