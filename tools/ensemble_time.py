#!/usr/bin/env python3
"""Closed-loop tracking ensemble about ONE optimum: aoc_track_ensemble against the replicated path it replaces.

    python tools/ensemble_time.py [--members 65536 262144] [--T 1000] [--seconds 0.5] [--repeats 3] [--out FILE]
                                  [--envelope] [--histogram] [--predict] [--lqg] [--filter] [--limits] [--lqg-limits]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ensemble_time.py --trace --members N
    python tools/ensemble_time.py --kernel-times DIR                 (kernel times: a traced run of its own, then its summary)

  A          aoc_lqr_tracking on the optimum replicated per member (gains + closed-loop rollout; states float32 in and out,
             the cheapest form of that path); its rollout kernel alone is k_track_rollout in the kernel trace
  B_stats    aoc_track_ensemble, statistics only         B_traj   ... writing x_reg (float32) and u_reg
  B_noise    ... statistics only, with the disturbance drawn on the device
--envelope adds the per-sample envelope over the members (aoc_track_ensemble_envelope, 44 numbers per sample):
  E_traj     the only way without it, part 1: aoc_track_ensemble writing x_reg and u_reg in fp64 (no dist_out)
  E_reduce   ... part 2: the same 44 numbers per sample from those arrays with torch, on the tiled device arrays as they
             lie (masked by first_bad; the moments as batched 6x64 by 64x6 fp64 products per tile and sample, summed over the
             tiles — the fastest of four forms tried, EXPERIMENTS.md)
  B_env      aoc_track_ensemble_envelope, statistics + envelope, no trajectories
and reports E = E_traj + E_reduce, B_env / E and B_env / B_stats (the price of the reduction).
--histogram adds the per-sample histogram over the members (aoc_track_ensemble_histogram, 8 x 64 counts per sample):
  H          aoc_track_ensemble_histogram, statistics + counts, no trajectories, under the bins of the envelope's min / max
  H_one_bin  the same call under bins with inv_w = 0: all 64 lanes of a tile add to ONE dword of LDS at every sample and
             channel, the worst case of the serialised adds
  Q_traj     the only way without it, part 1: aoc_track_ensemble writing x_reg and u_reg in fp64 (no dist_out)
  Q_count    ... part 2, the same counts with torch on the tiled device arrays: the bin of every value, then one
             scatter_add_ of ones per 256 tiles
  Q_sort     ... part 2 the other way, the three quantiles 0.05 / 0.5 / 0.95 themselves: torch.quantile over the members
             of dx and du (a sort per sample and channel), no mask for members that left
and reports C = B_stats, E = B_env, Q = Q_traj + min(Q_count, Q_sort), H/C, H/E and H/Q; --hist-valu, the vector
instructions of one stage of the H kernel from the ISA, gives its share of the vector-issue roof as --valu does for B_stats.
--predict adds the linear covariance prediction (aoc_track_covariance, 32 numbers per sample and optimum), for n_opt = 1, 64
and 1024 windows of the optimum (--T at most 800 leaves room for them; otherwise the optimum is repeated):
  P_n        aoc_track_covariance for n optima (both kernels)
  TQ_n       the best torch route to the same 32 numbers: Jacobians from aoc_step_batch for all (optimum, stage) pairs, then
             a stage loop of batched fp64 matmuls on the device (F P F^T + W, F m + c, K m, K P K^T)
against B_stats and B_env of the same run (the cheapest Monte-Carlo answers), and the quantile route on the device: two
passes B_env + H against one pass P_1 + H.
--lqg adds the loop with noisy measurements and a Kalman estimate (aoc_track_ensemble_lqg, statistics only, both kernels;
gains from batch.filter_gains, rho = 0.1 of the members' spread):
  L_plain    no disturbance and no measurement noise drawn (against B_stats)
  L_noise    the disturbance and the measurement noise drawn on the device (against B_noise)
and reports L_noise / B_noise and L_plain / B_stats of the same run.
--filter adds the filter Riccati recursion on the device (aoc_filter_gains, both kernels, gains only: cov = NULL), for n_opt =
1, 64 and 1024 windows of the optimum as --predict takes them, prior diag(DELTA_SCALE^2), rho = 0.1 of it, all six channels:
  G_n        aoc_filter_gains for n optima
  P_n        aoc_track_covariance for n optima in the same run: the same chain without the downdates
and reports G_n / P_n, and the host recursion batch.filter_gains for ONE optimum with the Jacobians already in hand (wall
clock, the median of three).
--joint adds the joint (dx, e) covariance prediction of the LQG loop (aoc_track_covariance_lqg, 96 numbers per sample and
optimum, all three kernels), for n_opt = 1, 64 and 1024 windows of the optimum as --predict takes them, the gains those of
aoc_filter_gains (prior diag(DELTA_SCALE^2), rho = 0.1 of it, all six channels), the prediction from the same prior:
  J_n        aoc_track_covariance_lqg for n optima, the gains already on the device
  JG_n       aoc_filter_gains, then aoc_track_covariance_lqg, on the same stream
  TJ_n       the best torch route to the same 96 numbers: Jacobians from aoc_step_batch for all (optimum, stage) pairs, then a
             stage loop of batched fp64 matmuls on the device
and reports J_n / P_n and J_n / G_n against the chains of --predict and --filter of the same run (give them too).
The optimum is the g4 fixture's (T = 1000; --T cuts it), the members are seeded perturbations of its first sample.
Profiler off: HIP events around at least --seconds of back-to-back launches per variant, after a warm-up of every variant;
the variants take turns inside each of --repeats rounds, so that a drift of the machine hits all of them.  One JSON line:
--limits adds the loop with actuator limits (aoc_track_ensemble_limited), statistics only, no disturbance:
  M_fixed    under the magnitude limits (-140, -260) .. (360, 430) and the rate limits (8200, 69000) per second of
             tests/test_limits_abi.py, no sat_count
  M_inf      under infinite limits (the outputs of B_stats, bit for bit), no sat_count
  M_count    as M_fixed, with sat_count (the tiles' counts and their fold)
and reports each over B_stats of the same run.
--lqg-limits adds the estimator's loop with actuator limits (aoc_track_ensemble_lqg_limited, statistics only, the fixed limits
of --limits, est_input = applied, no sat_count) beside the variants of --lqg, which it implies:
  N_plain    no disturbance and no measurement noise drawn (against L_plain)
  N_noise    both drawn on the device (against L_noise)
and reports N_plain / L_plain and N_noise / L_noise of the same run.
per size and variant the ms per call of every round, B/A, member-stages per second, and — from --valu, the vector
instructions of one stage on the executed path of the ISA (tools/one_kernel.sh, tools/isa_loops.py) — the share of the fp64
vector-issue roof (1024 SIMDs, one instruction per 4 cycles at 2.4 GHz): this kernel's bound is issue, not HBM.
--trace: three calls per variant and size and nothing else, for the kernel trace; --kernel-times DIR (no GPU) then reads
the *kernel_trace.csv under DIR and prints per tracking kernel its durations, their median and spread.  An allocation the
device refuses is reported for that size, never shrunk."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SIMDS, CYCLES_PER_VALU, CLOCK_HZ = 1024, 4, 2.4e9
DELTA_SCALE = np.array([0.3, 0.3, 0.5, 0.05, 0.1, 0.05])
SIGMA = np.array([1e-3, 1e-3, 1e-2, 1e-4, 1e-3, 1e-4])


def setup(B, T, g, envelope=False, histogram=False, lqg=False, limits=False, lqg_limits=False):
    """Device buffers and the launch closures for B members."""
    import torch
    from aircraftoptimalcontrol_amd import _lib, batch
    from aircraftoptimalcontrol_amd.batch import TILE, _ptr, alloc_tiled, check, lib, ntiles, pack, pack_vec
    dev = torch.device("cuda:0")
    xo, uo = g["xx_opt"][:, :T], g["uu_opt"][:, :T]
    bp = batch.BatchProblem(g["QQt"], g["RRt"], g["QQT"], np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]), device=dev)
    nt = ntiles(B)
    rng = np.random.default_rng(3)
    x0 = xo[:, 0] + rng.normal(size=(B, 6)) * DELTA_SCALE
    x0t = pack_vec(x0, dev)
    status = torch.zeros(nt * TILE, dtype=torch.int32, device=dev)
    # A: one tile of the optimum, replicated over the tiles on the device
    rep = lambda a, f32=False: pack(np.repeat(a[None], TILE, 0), dev, f32=f32).expand(nt, -1, -1, -1).contiguous()
    xt, ut = rep(xo, True), rep(uo)
    xo0 = pack_vec(np.repeat(xo[:, 0][None], B, 0), dev)
    Kg = alloc_tiled(B, T, 12, dev)
    xr, ur = alloc_tiled(B, T, 6, dev, f32=True), alloc_tiled(B, T, 2, dev)
    pA = bp.c_problem(B, x_in_f32=1, x_out_f32=1)

    def run_A():
        check(lib().aoc_lqr_tracking(C.byref(pA), _ptr(xt), _ptr(ut), _ptr(xo0), _ptr(x0t), _ptr(Kg), _ptr(xr), _ptr(ur),
                                     _ptr(status)), "aoc_lqr_tracking")

    # B: the gains of ONE trajectory, the nominal once
    KK, _ = batch.tracking_gains(bp, xo[None], uo[None])
    nominal = torch.from_numpy(batch.ensemble_nominal(xo[None], uo[None], KK)).to(dev)
    stats = torch.empty((nt, batch.ENS_NSTAT, TILE), dtype=torch.float64, device=dev)
    nz = _lib.MpcNoise(20261016, 0, 0, (C.c_double * 6)(*SIGMA.tolist()))
    pB = bp.c_problem(B, x_out_f32=1)

    def run_B(traj=False, noise=False):
        check(lib().aoc_track_ensemble(C.byref(pB), 1, nt * TILE, _ptr(nominal), _ptr(x0t), C.byref(nz) if noise else None,
                                       _ptr(xr) if traj else None, _ptr(ur) if traj else None, None, _ptr(stats),
                                       _ptr(status)), "aoc_track_ensemble")

    runs = dict(A=run_A, B_stats=run_B, B_traj=lambda: run_B(traj=True), B_noise=lambda: run_B(noise=True))
    if lqg:
        rho = 0.1 * DELTA_SCALE
        Lf = batch.filter_gains(bp, xo, uo, np.diag(DELTA_SCALE ** 2), SIGMA, rho)[0]
        filt = torch.from_numpy(np.ascontiguousarray(Lf.reshape(36, T).T)[None]).to(dev)        # [1][T][36]
        est_stats = torch.empty((nt, batch.LQG_NSTAT, TILE), dtype=torch.float64, device=dev)
        nbytes = int(lib().aoc_track_ensemble_lqg_scratch_bytes(1, T))
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        rho_c = (C.c_double * 6)(*rho.tolist())

        def run_L(noise=False):
            check(lib().aoc_track_ensemble_lqg(C.byref(pB), 1, nt * TILE, _ptr(nominal), _ptr(filt), _ptr(x0t), None,
                                               C.byref(nz) if noise else None, rho_c if noise else None, None, None, None, None,
                                               None, _ptr(stats), _ptr(est_stats), _ptr(status), _ptr(scratch), nbytes),
                  "aoc_track_ensemble_lqg")

        runs.update(L_plain=run_L, L_noise=lambda: run_L(noise=True))
        if lqg_limits:
            two = lambda a, b: (C.c_double * 2)(a, b)
            lfixed = _lib.ActuatorLimits(two(-140.0, -260.0), two(360.0, 430.0), two(8200.0, 69000.0))
            lsat = torch.empty((nt, batch.SAT_NSTAT, TILE), dtype=torch.float64, device=dev)
            nlbytes = int(lib().aoc_track_ensemble_lqg_limited_scratch_bytes(B, 1, T, nt * TILE, 0))
            assert nlbytes == nbytes

            def run_N(noise=False):
                check(lib().aoc_track_ensemble_lqg_limited(C.byref(pB), 1, nt * TILE, _ptr(nominal), _ptr(filt), _ptr(x0t), None,
                                                           C.byref(nz) if noise else None, rho_c if noise else None,
                                                           C.byref(lfixed), _lib.EST_INPUT_APPLIED, None, None, None, None, None,
                                                           _ptr(stats), _ptr(est_stats), _ptr(lsat), None, _ptr(status),
                                                           _ptr(scratch), nbytes), "aoc_track_ensemble_lqg_limited")

            runs.update(N_plain=run_N, N_noise=lambda: run_N(noise=True))
    if limits:
        inf = float("inf")
        two = lambda a, b: (C.c_double * 2)(a, b)
        fixed = _lib.ActuatorLimits(two(-140.0, -260.0), two(360.0, 430.0), two(8200.0, 69000.0))
        none = _lib.ActuatorLimits(two(-inf, -inf), two(inf, inf), two(inf, inf))
        sat = torch.empty((nt, batch.SAT_NSTAT, TILE), dtype=torch.float64, device=dev)
        sat_count = torch.empty((1, T, 2), dtype=torch.int32, device=dev)
        mbytes = int(lib().aoc_ensemble_limited_scratch_bytes(_lib.ENS_MODE_STATS, B, T, nt * TILE, 1))
        mscratch = torch.empty(mbytes // 8, dtype=torch.float64, device=dev)

        def run_M(lim, count=False):
            check(lib().aoc_track_ensemble_limited(C.byref(pB), _lib.ENS_MODE_STATS, 1, nt * TILE, _ptr(nominal), _ptr(x0t), None,
                                                   C.byref(lim), None, None, None, None, _ptr(stats), _ptr(status), _ptr(sat),
                                                   _ptr(sat_count) if count else None, None, None,
                                                   _ptr(mscratch) if count else None, mbytes if count else 0),
                  "aoc_track_ensemble_limited")

        runs.update(M_fixed=lambda: run_M(fixed), M_inf=lambda: run_M(none), M_count=lambda: run_M(fixed, True))
    if not envelope and not histogram:
        return runs
    # E: trajectories in fp64 + a torch reduction on the tiled arrays [tile][t][c][lane]
    xr64, ur64 = alloc_tiled(B, T, 6, dev), alloc_tiled(B, T, 2, dev)
    pE = bp.c_problem(B)
    xo_d, uo_d = nominal[0, :, 0:6], nominal[0, :, 6:8]   # (T,6), (T,2)
    tt = torch.arange(T, device=dev)
    inf = float("inf")
    live = (torch.arange(nt * TILE, device=dev) < B).view(nt, 1, TILE)

    def run_E_traj():
        check(lib().aoc_track_ensemble(C.byref(pE), 1, nt * TILE, _ptr(nominal), _ptr(x0t), None, _ptr(xr64), _ptr(ur64), None,
                                       _ptr(stats), _ptr(status)), "aoc_track_ensemble")

    def run_E_reduce():
        xv, uv = xr64.view(nt, T, 6, TILE), ur64.view(nt, T, 2, TILE)
        counts = (tt.view(1, T, 1) < stats[:, 15, :].view(nt, 1, TILE)) & live       # (nt,T,64)
        c4 = counts.unsqueeze(2)
        dx, du = xv - xo_d.view(1, T, 6, 1), uv - uo_d.view(1, T, 2, 1)
        rec = torch.empty((T, 44), dtype=torch.float64, device=dev)
        rec[:, 0] = counts.sum(dim=(0, 2))
        rec[:, 1:7] = torch.where(c4, dx, inf).amin(dim=(0, 3))
        rec[:, 7:13] = torch.where(c4, dx, -inf).amax(dim=(0, 3))
        rec[:, 13:15] = torch.where(c4, du, inf).amin(dim=(0, 3))
        rec[:, 15:17] = torch.where(c4, du, -inf).amax(dim=(0, 3))
        rec[T - 1, 13:15], rec[T - 1, 15:17] = inf, -inf
        dz = torch.where(c4, dx, 0.0)
        rec[:, 17:23] = dz.sum(dim=(0, 3))
        mom = torch.zeros((T, 6, 6), dtype=torch.float64, device=dev)
        for i in range(0, nt, 128):          # 6x64 by 64x6 per (tile, sample), then over the tiles: the fastest form tried
            d = dz[i:i + 128]                # (one batched product over all members, K = B: 42 ms at 65 536; pair by pair: 12)
            mom += torch.matmul(d, d.transpose(2, 3)).sum(dim=0)
        iu = torch.triu_indices(6, 6, device=dev)
        rec[:, 23:44] = mom[:, iu[0], iu[1]]
        return rec

    env = torch.empty((1, T, _lib.AOC_ENV_NREC), dtype=torch.float64, device=dev)
    nbytes = int(lib().aoc_ensemble_envelope_scratch_bytes(B, T, nt * TILE))
    scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)

    def run_B_env():
        check(lib().aoc_track_ensemble_envelope(C.byref(pB), 1, nt * TILE, _ptr(nominal), _ptr(x0t), None, None, None, None,
                                                _ptr(stats), _ptr(status), _ptr(env), _ptr(scratch), nbytes),
              "aoc_track_ensemble_envelope")

    # the two ways agree before either is timed (n, min, max exactly; the sums to 1e-9 of their scale: a plausibility
    # check of the yardstick, the tests hold the bound)
    run_E_traj(); want = run_E_reduce(); run_B_env(); torch.cuda.synchronize()
    got = env[0]
    assert torch.equal(got[:, :17], want[:, :17]), "E and B_env disagree in n / min / max"
    assert bool(((got[:, 17:] - want[:, 17:]).abs() <= 1e-9 * want[:, 17:].abs().max()).all()), "E and B_env disagree in the sums"
    if envelope:
        runs.update(E_traj=run_E_traj, E_reduce=run_E_reduce)
    runs.update(B_env=run_B_env)
    if not histogram:
        return runs
    # H: the second pass under the bins of the first; Q: trajectories in fp64 + torch, to the same counts or to quantiles
    NCH, NBIN = _lib.AOC_HIST_NCH, _lib.AOC_HIST_NBIN
    bins = torch.from_numpy(batch.histogram_bins(env.cpu().numpy())).to(dev)                  # (1,T,8,2)
    hist = torch.empty((1, T, NCH, NBIN), dtype=torch.int32, device=dev)
    hbytes = int(lib().aoc_ensemble_histogram_scratch_bytes(B, T, nt * TILE))
    hscratch = torch.empty(max(hbytes, 8) // 8, dtype=torch.float64, device=dev)

    def run_H():
        check(lib().aoc_track_ensemble_histogram(C.byref(pB), 1, nt * TILE, _ptr(nominal), _ptr(x0t), None, _ptr(bins), None, None,
                                                 None, _ptr(stats), _ptr(status), _ptr(hist), _ptr(hscratch), hbytes),
              "aoc_track_ensemble_histogram")

    bins_one = bins.clone()
    bins_one[..., 1] = 0.0
    hist_one = torch.empty_like(hist)

    def run_H_one_bin():
        check(lib().aoc_track_ensemble_histogram(C.byref(pB), 1, nt * TILE, _ptr(nominal), _ptr(x0t), None, _ptr(bins_one), None,
                                                 None, None, _ptr(stats), _ptr(status), _ptr(hist_one), _ptr(hscratch), hbytes),
              "aoc_track_ensemble_histogram")

    lo, inv_w = bins[0, :, :, 0].contiguous(), bins[0, :, :, 1].contiguous()                  # (T,8)
    slot = (torch.arange(T, device=dev, dtype=torch.int32).view(1, T, 1, 1) * NCH
            + torch.arange(NCH, device=dev, dtype=torch.int32).view(1, 1, NCH, 1)) * NBIN     # (1,T,8,1)
    dump = T * NCH * NBIN                                                                     # where what does not count goes
    CH = 256

    def run_Q_count():
        xv, uv = xr64.view(nt, T, 6, TILE), ur64.view(nt, T, 2, TILE)
        acc = torch.zeros(dump + 1, dtype=torch.int32, device=dev)
        for i in range(0, nt, CH):
            v = torch.cat([xv[i:i + CH] - xo_d.view(1, T, 6, 1), uv[i:i + CH] - uo_d.view(1, T, 2, 1)], dim=2)   # (ch,T,8,64)
            s = (v - lo.view(1, T, NCH, 1)) * inv_w.view(1, T, NCH, 1)
            k = torch.where(s >= 63.0, 63.0, torch.where(s >= 1.0, s, 0.0)).to(torch.int32)
            counts = ((tt.view(1, T, 1) < stats[i:i + CH, 15, :].view(-1, 1, TILE)) & live[i:i + CH]).unsqueeze(2)
            idx = torch.where(counts, slot + k, dump)
            idx[:, T - 1, 6:, :] = dump
            acc.scatter_add_(0, idx.view(-1).to(torch.int64), torch.ones((), dtype=torch.int32, device=dev).expand(idx.numel()))
        return acc[:dump].view(T, NCH, NBIN)

    qq = torch.tensor([0.05, 0.5, 0.95], dtype=torch.float64, device=dev)

    def run_Q_sort():
        xv, uv = xr64.view(nt, T, 6, TILE), ur64.view(nt, T, 2, TILE)
        out = torch.empty((3, T, NCH), dtype=torch.float64, device=dev)
        for c in range(NCH):          # channel by channel: one (T, members) array at a time
            v = (xv[:, :, c, :] - xo_d[:, c].view(1, T, 1)) if c < 6 else (uv[:, :, c - 6, :] - uo_d[:, c - 6].view(1, T, 1))
            v = v.permute(1, 0, 2).reshape(T, nt * TILE)
            out[:, :, c] = torch.sort(v, dim=1).values[:, ((qq * (nt * TILE)).ceil().clamp(min=1) - 1).long()].T
        return out

    # the two ways to the counts agree before either is timed
    run_E_traj(); want = run_Q_count(); run_H(); torch.cuda.synchronize()
    assert torch.equal(hist[0], want), "Q_count and H disagree"
    run_H_one_bin(); torch.cuda.synchronize()
    assert int(hist_one[..., 0].sum()) == int(hist_one.sum()) == int(hist.sum()), "H_one_bin: not everything in bin 0"
    runs.update(H=run_H, H_one_bin=run_H_one_bin, Q_traj=run_E_traj, Q_count=run_Q_count, Q_sort=run_Q_sort)
    return runs


def setup_filter(T, g, sizes=(1, 64, 1024)):
    """Launch closures of aoc_filter_gains for each n_opt in `sizes`, and the host recursion's time for one optimum [ms]."""
    import time
    import torch
    from aircraftoptimalcontrol_amd import _lib, batch
    from aircraftoptimalcontrol_amd.batch import _ptr, check, lib
    dev = torch.device("cuda:0")
    Tg = g["xx_opt"].shape[1]
    bp = batch.BatchProblem(g["QQt"], g["RRt"], g["QQT"], np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]), device=dev)
    nz = _lib.MpcNoise(20261016, 0, 0, (C.c_double * 6)(*SIGMA.tolist()))
    rho = 0.1 * DELTA_SCALE
    rho_c = (C.c_double * 6)(*rho.tolist())
    S0 = torch.from_numpy(np.diag(DELTA_SCALE ** 2)[np.triu_indices(6)]).to(dev)
    runs, filts = {}, {}
    for n in sizes:
        off = [(k % max(1, Tg - T + 1)) for k in range(n)]
        xo = np.stack([g["xx_opt"][:, o:o + T] for o in off])
        uo = np.stack([g["uu_opt"][:, o:o + T] for o in off])
        nominal = torch.from_numpy(batch.ensemble_nominal(xo, uo, np.zeros((n, 2, 6, T)))).to(dev)
        Sig = S0.repeat(n, 1).contiguous()
        filt = torch.empty((n, T, 36), dtype=torch.float64, device=dev)
        nbytes = int(lib().aoc_filter_gains_scratch_bytes(n, T))
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        p = bp.c_problem(n)

        def run_G(p=p, n=n, nominal=nominal, Sig=Sig, filt=filt, scratch=scratch, nbytes=nbytes):
            check(lib().aoc_filter_gains(C.byref(p), n, _ptr(nominal), _ptr(Sig), C.byref(nz), rho_c, 63, _ptr(filt), None, None,
                                         _ptr(scratch), nbytes), "aoc_filter_gains")

        runs["G_%d" % n], filts[n] = run_G, filt
    xo, uo = g["xx_opt"][:, :T], g["uu_opt"][:, :T]
    fx = batch.step_batch(bp.model, xo[:, :T - 1].T, uo[:, :T - 1].T, device=dev)[1]
    A = fx.transpose(0, 2, 1)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        Lh = batch.filter_gains(bp, xo, uo, np.diag(DELTA_SCALE ** 2), SIGMA, rho, jac=(A, None))[0]
        host.append((time.perf_counter() - t0) * 1e3)
    n0 = sizes[0]                                                                        # window 0: the two agree before either is timed
    runs["G_%d" % n0](); torch.cuda.synchronize()
    got = filts[n0][0].cpu().numpy().reshape(T, 6, 6).transpose(1, 2, 0)
    assert np.abs(got - Lh).max() <= 1e-9 * np.abs(Lh).max(), "aoc_filter_gains and filter_gains disagree"
    return runs, float(np.median(host))


def setup_predict(T, g, sizes=(1, 64, 1024), torch_route=True):
    """Launch closures of the prediction for each n_opt in `sizes`, and of the torch route to the same records."""
    import torch
    from aircraftoptimalcontrol_amd import _lib, batch
    from aircraftoptimalcontrol_amd.batch import _ptr, check, lib
    dev = torch.device("cuda:0")
    Tg = g["xx_opt"].shape[1]
    bp = batch.BatchProblem(g["QQt"], g["RRt"], g["QQT"], np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]), device=dev)
    nz = _lib.MpcNoise(20261016, 0, 0, (C.c_double * 6)(*SIGMA.tolist()))
    S0 = torch.from_numpy(np.diag((0.1 * DELTA_SCALE) ** 2)[np.triu_indices(6)]).to(dev)
    runs = {}
    for n in sizes:
        off = [(k % max(1, Tg - T + 1)) for k in range(n)]
        xo = np.stack([g["xx_opt"][:, o:o + T] for o in off])
        uo = np.stack([g["uu_opt"][:, o:o + T] for o in off])
        KK = np.stack([g["KK"][:, :, o:o + T] for o in off])
        nominal = torch.from_numpy(batch.ensemble_nominal(xo, uo, KK)).to(dev)
        Sig = S0.repeat(n, 1).contiguous()
        pred = torch.empty((n, T, _lib.AOC_COV_NREC), dtype=torch.float64, device=dev)
        nbytes = int(lib().aoc_track_covariance_scratch_bytes(n, T))
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        p = bp.c_problem(n)

        def run_P(p=p, n=n, nominal=nominal, Sig=Sig, pred=pred, scratch=scratch, nbytes=nbytes):
            check(lib().aoc_track_covariance(C.byref(p), n, _ptr(nominal), None, _ptr(Sig), C.byref(nz), _ptr(pred), None,
                                             _ptr(scratch), nbytes), "aoc_track_covariance")

        # the torch route: one aoc_step_batch over all pairs, then T-1 dependent stages of batched 6x6 products
        xs = nominal[:, :, 0:6].reshape(-1, 6).contiguous()
        us = nominal[:, :, 6:8].reshape(-1, 2).contiguous()
        Kt = nominal[:, :, 8:20].reshape(n, T, 2, 6)
        xp = torch.empty((n * T, 6), dtype=torch.float64, device=dev)
        fx = torch.empty((n * T, 6, 6), dtype=torch.float64, device=dev)
        fu = torch.empty((n * T, 2, 6), dtype=torch.float64, device=dev)
        W = torch.diag(torch.from_numpy(SIGMA ** 2)).to(dev)
        iu = torch.triu_indices(6, 6, device=dev)
        P0 = torch.zeros((n, 6, 6), dtype=torch.float64, device=dev)
        P0[:, iu[0], iu[1]] = Sig
        P0 = P0 + P0.transpose(1, 2) - torch.diag_embed(torch.diagonal(P0, dim1=1, dim2=2))
        out = torch.zeros((n, T, _lib.AOC_COV_NREC), dtype=torch.float64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def run_TQ(n=n, xs=xs, us=us, Kt=Kt, xp=xp, fx=fx, fu=fu, P0=P0, out=out, nominal=nominal):
            check(lib().aoc_step_batch(C.byref(bp.model), n * T, _ptr(xs), _ptr(us), None, _ptr(xp), _ptr(fx), _ptr(fu), None, None,
                                       None, st), "aoc_step_batch")
            A = fx.view(n, T, 6, 6).transpose(2, 3)
            Bm = fu.view(n, T, 2, 6).transpose(2, 3)
            F = A + torch.matmul(Bm, Kt)                                                # (n,T,6,6)
            c = xp.view(n, T, 6)[:, :T - 1] - nominal[:, 1:, 0:6]
            P, m = P0, torch.zeros((n, 6, 1), dtype=torch.float64, device=dev)
            for t in range(T):
                out[:, t, 0:6] = m[:, :, 0]
                out[:, t, 6:27] = P[:, iu[0], iu[1]]
                if t == T - 1:
                    break
                KP = torch.matmul(Kt[:, t], P)
                out[:, t, 27:29] = torch.matmul(Kt[:, t], m)[:, :, 0]
                KPK = torch.matmul(KP, Kt[:, t].transpose(1, 2))
                out[:, t, 29], out[:, t, 30], out[:, t, 31] = KPK[:, 0, 0], KPK[:, 0, 1], KPK[:, 1, 1]
                m = torch.matmul(F[:, t], m) + c[:, t].unsqueeze(2)
                P = torch.matmul(torch.matmul(F[:, t], P), F[:, t].transpose(1, 2)) + W
            return out

        runs["P_%d" % n] = run_P
        if not torch_route:
            continue
        run_P(); want = run_TQ(); torch.cuda.synchronize()                                # the two routes agree before either is timed
        scale = want.abs().amax(dim=(0, 1)).clamp(min=1e-300)
        assert bool((((pred - want).abs() / scale) <= 1e-9).all()), "P and TQ disagree"
        runs["TQ_%d" % n] = run_TQ
    return runs


def setup_joint(T, g, sizes=(1, 64, 1024), torch_route=True):
    """Launch closures of the joint prediction for each n_opt in `sizes`: with the gains in hand, with aoc_filter_gains in front,
    and of the torch route to the same records."""
    import torch
    from aircraftoptimalcontrol_amd import _lib, batch
    from aircraftoptimalcontrol_amd.batch import _ptr, check, lib
    dev = torch.device("cuda:0")
    Tg = g["xx_opt"].shape[1]
    bp = batch.BatchProblem(g["QQt"], g["RRt"], g["QQT"], np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]), device=dev)
    nz = _lib.MpcNoise(20261016, 0, 0, (C.c_double * 6)(*SIGMA.tolist()))
    rho = 0.1 * DELTA_SCALE
    rho_c = (C.c_double * 6)(*rho.tolist())
    S0 = torch.from_numpy(np.diag(DELTA_SCALE ** 2)[np.triu_indices(6)]).to(dev)
    NREC = _lib.AOC_LQGCOV_NREC
    runs = {}
    for n in sizes:
        off = [(k % max(1, Tg - T + 1)) for k in range(n)]
        xo = np.stack([g["xx_opt"][:, o:o + T] for o in off])
        uo = np.stack([g["uu_opt"][:, o:o + T] for o in off])
        KK = np.stack([g["KK"][:, :, o:o + T] for o in off])
        nominal = torch.from_numpy(batch.ensemble_nominal(xo, uo, KK)).to(dev)
        Sig = S0.repeat(n, 1).contiguous()
        filt = torch.empty((n, T, 36), dtype=torch.float64, device=dev)
        pred = torch.empty((n, T, NREC), dtype=torch.float64, device=dev)
        gbytes = int(lib().aoc_filter_gains_scratch_bytes(n, T))
        nbytes = int(lib().aoc_track_covariance_lqg_scratch_bytes(n, T))
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        p = bp.c_problem(n)

        def run_G(p=p, n=n, nominal=nominal, Sig=Sig, filt=filt, scratch=scratch, gbytes=gbytes):
            check(lib().aoc_filter_gains(C.byref(p), n, _ptr(nominal), _ptr(Sig), C.byref(nz), rho_c, 63, _ptr(filt), None, None,
                                         _ptr(scratch), gbytes), "aoc_filter_gains")

        def run_J(p=p, n=n, nominal=nominal, Sig=Sig, filt=filt, pred=pred, scratch=scratch, nbytes=nbytes):
            check(lib().aoc_track_covariance_lqg(C.byref(p), n, _ptr(nominal), _ptr(filt), None, None, _ptr(Sig), C.byref(nz), rho_c,
                                                 _ptr(pred), None, _ptr(scratch), nbytes), "aoc_track_covariance_lqg")

        def run_JG(run_G=run_G, run_J=run_J):
            run_G()
            run_J()

        run_G()
        runs["J_%d" % n], runs["JG_%d" % n] = run_J, run_JG
        if not torch_route:
            continue
        # the torch route: one aoc_step_batch over all pairs, then T dependent stages of batched 6x6 products
        xs = nominal[:, :, 0:6].reshape(-1, 6).contiguous()
        us = nominal[:, :, 6:8].reshape(-1, 2).contiguous()
        Kt = nominal[:, :, 8:20].reshape(n, T, 2, 6)
        xp = torch.empty((n * T, 6), dtype=torch.float64, device=dev)
        fx = torch.empty((n * T, 6, 6), dtype=torch.float64, device=dev)
        fu = torch.empty((n * T, 2, 6), dtype=torch.float64, device=dev)
        W = torch.diag(torch.from_numpy(SIGMA ** 2)).to(dev)
        V = torch.diag(torch.from_numpy(rho ** 2)).to(dev)
        I6 = torch.eye(6, dtype=torch.float64, device=dev)
        iu = torch.triu_indices(6, 6, device=dev)
        P0 = torch.zeros((n, 6, 6), dtype=torch.float64, device=dev)
        P0[:, iu[0], iu[1]] = Sig
        P0 = P0 + P0.transpose(1, 2) - torch.diag_embed(torch.diagonal(P0, dim1=1, dim2=2))
        out = torch.zeros((n, T, NREC), dtype=torch.float64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def run_TJ(n=n, xs=xs, us=us, Kt=Kt, xp=xp, fx=fx, fu=fu, P0=P0, out=out, nominal=nominal, filt=filt):
            check(lib().aoc_step_batch(C.byref(bp.model), n * T, _ptr(xs), _ptr(us), None, _ptr(xp), _ptr(fx), _ptr(fu), None, None,
                                       None, st), "aoc_step_batch")
            A = fx.view(n, T, 6, 6).transpose(2, 3)
            N = torch.matmul(fu.view(n, T, 2, 6).transpose(2, 3), Kt)                   # (n,T,6,6)
            F = A + N
            Lt = filt.view(n, T, 6, 6)
            J = I6 - Lt
            LVL = torch.matmul(torch.matmul(Lt, V), Lt.transpose(2, 3))                 # off the chain, all samples at once
            c = xp.view(n, T, 6)[:, :T - 1] - nominal[:, 1:, 0:6]
            z = torch.zeros((n, 6, 1), dtype=torch.float64, device=dev)
            X, Cm, Em, m, mu = P0, P0, P0, z, z
            for t in range(T):
                Jt = J[:, t]
                mu = torch.matmul(Jt, mu)
                E = torch.matmul(torch.matmul(Jt, Em), Jt.transpose(1, 2)) + LVL[:, t]
                Cx = torch.matmul(Cm, Jt.transpose(1, 2))
                out[:, t, 0:6], out[:, t, 6:12] = m[:, :, 0], mu[:, :, 0]
                out[:, t, 12:33], out[:, t, 33:54] = X[:, iu[0], iu[1]], E[:, iu[0], iu[1]]
                out[:, t, 54:90] = Cx.reshape(n, 36)
                if t == T - 1:
                    break
                K = Kt[:, t]
                out[:, t, 90:92] = torch.matmul(K, m - mu)[:, :, 0]
                KHK = torch.matmul(torch.matmul(K, X - Cx - Cx.transpose(1, 2) + E), K.transpose(1, 2))
                out[:, t, 92], out[:, t, 93], out[:, t, 94] = KHK[:, 0, 0], KHK[:, 0, 1], KHK[:, 1, 1]
                Ft, Nt, At = F[:, t], N[:, t], A[:, t]
                Y1 = torch.matmul(Ft, X) - torch.matmul(Nt, Cx.transpose(1, 2))
                Y2 = torch.matmul(Ft, Cx) - torch.matmul(Nt, E)
                m = torch.matmul(Ft, m) - torch.matmul(Nt, mu) + c[:, t].unsqueeze(2)
                mu = torch.matmul(At, mu)
                X = torch.matmul(Y1, Ft.transpose(1, 2)) - torch.matmul(Y2, Nt.transpose(1, 2)) + W
                Cm = torch.matmul(Y2, At.transpose(1, 2)) + W
                Em = torch.matmul(torch.matmul(At, E), At.transpose(1, 2)) + W
            return out

        run_J(); want = run_TJ(); torch.cuda.synchronize()                                # the two routes agree before either is timed
        scale = want.abs().amax(dim=(0, 1)).clamp(min=1e-300)
        assert bool((((pred - want).abs() / scale) <= 1e-8).all()), "J and TJ disagree"
        runs["TJ_%d" % n] = run_TJ
    return runs


def timed(fn, seconds):
    """ms per call over at least `seconds` of back-to-back launches (HIP events; one launch first sizes the window)"""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(); fn(); ev[1].record(); torch.cuda.synchronize()
    n = max(2, int(np.ceil(seconds * 1e3 / max(ev[0].elapsed_time(ev[1]), 1e-3))))
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record(); torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n, n


def kernel_times(d):
    """Durations [ms] of the tracking kernels in the rocprofv3 kernel trace(s) under d, in launch order: *kernel_trace.csv
    (--output-format csv) or the *_results.db this rocprofv3 writes by default (its `kernels` view)."""
    import collections
    import csv
    import glob
    import sqlite3
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Grid_Size_X", r.get("Grid_Size", "?")))
                 for r in csv.DictReader(open(f))]
    if not rows:
        for f in sorted(glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)):
            rows += list(sqlite3.connect(f).execute("select name, start, end, grid_x from kernels"))
    out = collections.OrderedDict()
    for name, t0, t1, grid in sorted(rows, key=lambda r: r[1]):
        name = name.split("(")[0].replace("void ", "").replace("aoc64::", "")
        if name.startswith(("k_track_", "k_envelope_", "k_histogram_", "k_cov_", "k_filter_", "k_lqgcov_", "k_sat_")):
            out.setdefault("%s grid=%s" % (name, grid), []).append(round((t1 - t0) / 1e6, 4))
    for k, v in out.items():
        print(json.dumps(dict(kernel=k, ms=v, median=float(np.median(v)), spread_rel=round((max(v) - min(v)) / float(np.median(v)), 4))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--valu", type=int, default=0, help="vector instructions per stage of the stats-only kernel (from the ISA)")
    ap.add_argument("--trace", action="store_true", help="three calls per variant and nothing else (under rocprofv3)")
    ap.add_argument("--kernel-times", default=None, metavar="DIR", help="summarise the kernel trace(s) under DIR (no GPU)")
    ap.add_argument("--envelope", action="store_true", help="also time the per-sample envelope: E_traj + E_reduce against B_env")
    ap.add_argument("--histogram", action="store_true", help="also time the per-sample histogram: H against B_stats, B_env and Q")
    ap.add_argument("--predict", action="store_true", help="also time aoc_track_covariance for 1, 64 and 1024 optima")
    ap.add_argument("--lqg", action="store_true", help="also time aoc_track_ensemble_lqg, statistics only, with and without draws")
    ap.add_argument("--filter", action="store_true", help="also time aoc_filter_gains for 1, 64 and 1024 optima")
    ap.add_argument("--joint", action="store_true", help="also time aoc_track_covariance_lqg for 1, 64 and 1024 optima")
    ap.add_argument("--limits", action="store_true", help="also time aoc_track_ensemble_limited, statistics only")
    ap.add_argument("--lqg-limits", action="store_true",
                    help="also time aoc_track_ensemble_lqg_limited against aoc_track_ensemble_lqg, statistics only")
    ap.add_argument("--hist-valu", type=int, default=0, help="vector instructions per stage of the histogram kernel (from the ISA)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_times:
        return kernel_times(a.kernel_times)
    import torch
    if not torch.cuda.is_available():
        sys.exit("ensemble_time.py needs the GPU: there is nothing to time without one")
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g4_lqr_tracking.npz"), allow_pickle=False))
    out = dict(T=a.T, seconds=a.seconds, sizes=[])
    for B in a.members:
        rec = dict(members=B)
        try:
            runs = setup(B, a.T, g, a.envelope, a.histogram or a.predict, a.lqg or a.lqg_limits, a.limits, a.lqg_limits)
            if a.predict:
                if not a.histogram:       # the yardsticks of the prediction only, not the torch routes to the histogram
                    runs = {k: f for k, f in runs.items() if k in ("A", "B_stats", "B_noise", "B_env", "H", "L_plain", "L_noise", "M_fixed", "M_inf", "M_count")}
                runs.update(setup_predict(a.T, g))
            if a.filter:
                if not a.predict:
                    runs.update(setup_predict(a.T, g, torch_route=False))
                filter_runs, host_ms = setup_filter(a.T, g)
                runs.update(filter_runs)
            if a.joint:
                runs.update(setup_joint(a.T, g))
        except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
            rec["refused"] = "allocation refused: %s" % str(e).split("\n")[0]
            out["sizes"].append(rec)
            continue
        for fn in runs.values():          # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        if a.trace:
            for fn in runs.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            rec["trace_calls_per_variant"] = 4
        else:
            ms = {k: [] for k in runs}
            for _ in range(a.repeats):
                for k, fn in runs.items():
                    ms[k].append(round(timed(fn, a.seconds)[0], 4))
            rec["ms"] = ms
            med = {k: float(np.median(v)) for k, v in ms.items()}
            rec["A_spread_rel"] = round((max(ms["A"]) - min(ms["A"])) / med["A"], 4)
            rec["B_over_A"] = {k: round(med[k] / med["A"], 4) for k in ms if k != "A"}
            if a.predict:
                sp = lambda k: round((max(ms[k]) - min(ms[k])) / med[k], 4)
                rec["predict"] = dict(P_ms={k: med[k] for k in med if k.startswith("P_")},
                                      TQ_ms={k: med[k] for k in med if k.startswith("TQ_")},
                                      C_ms=med["B_stats"], E_ms=med["B_env"], H_ms=med["H"],
                                      P1_over_C=round(med["P_1"] / med["B_stats"], 4),
                                      two_pass_ms=round(med["B_env"] + med["H"], 4), one_pass_ms=round(med["P_1"] + med["H"], 4),
                                      spread_rel={k: sp(k) for k in ("P_1", "P_64", "P_1024", "B_stats", "B_env", "H")})
            if a.lqg:
                sp = lambda k: round((max(ms[k]) - min(ms[k])) / med[k], 4)
                rec["lqg"] = dict(L_plain_ms=med["L_plain"], L_noise_ms=med["L_noise"], B_stats_ms=med["B_stats"],
                                  B_noise_ms=med["B_noise"], L_noise_over_B_noise=round(med["L_noise"] / med["B_noise"], 4),
                                  L_plain_over_B_stats=round(med["L_plain"] / med["B_stats"], 4),
                                  spread_rel={k: sp(k) for k in ("L_plain", "L_noise", "B_stats", "B_noise")})
            if a.lqg_limits:
                sp = lambda k: round((max(ms[k]) - min(ms[k])) / med[k], 4)
                ks = ("N_plain", "N_noise", "L_plain", "L_noise")
                rec["lqg_limits"] = dict(**{k + "_ms": med[k] for k in ks},
                                         N_plain_over_L_plain=round(med["N_plain"] / med["L_plain"], 4),
                                         N_noise_over_L_noise=round(med["N_noise"] / med["L_noise"], 4),
                                         spread_rel={k: sp(k) for k in ks})
            if a.limits:
                sp = lambda k: round((max(ms[k]) - min(ms[k])) / med[k], 4)
                ks = ("M_fixed", "M_inf", "M_count")
                rec["limits"] = dict(B_stats_ms=med["B_stats"], **{k + "_ms": med[k] for k in ks},
                                     **{k + "_over_B_stats": round(med[k] / med["B_stats"], 4) for k in ks},
                                     spread_rel={k: sp(k) for k in ks + ("B_stats",)})
            if a.filter:
                sp = lambda k: round((max(ms[k]) - min(ms[k])) / med[k], 4)
                ns = (1, 64, 1024)
                rec["filter"] = dict(G_ms={"G_%d" % n: med["G_%d" % n] for n in ns}, P_ms={"P_%d" % n: med["P_%d" % n] for n in ns},
                                     G_over_P={n: round(med["G_%d" % n] / med["P_%d" % n], 4) for n in ns},
                                     host_one_optimum_ms=round(host_ms, 3), host_over_G_1=round(host_ms / med["G_1"], 1),
                                     spread_rel={k: sp(k) for n in ns for k in ("G_%d" % n, "P_%d" % n)})
            if a.joint:
                sp = lambda k: round((max(ms[k]) - min(ms[k])) / med[k], 4)
                ns = (1, 64, 1024)
                rec["joint"] = dict(J_ms={"J_%d" % n: med["J_%d" % n] for n in ns}, JG_ms={"JG_%d" % n: med["JG_%d" % n] for n in ns},
                                    TJ_ms={"TJ_%d" % n: med["TJ_%d" % n] for n in ns},
                                    TJ_over_J={n: round(med["TJ_%d" % n] / med["J_%d" % n], 1) for n in ns},
                                    spread_rel={k: sp(k) for n in ns for k in ("J_%d" % n, "JG_%d" % n)})
                if "P_1" in med:
                    rec["joint"]["J_over_P"] = {n: round(med["J_%d" % n] / med["P_%d" % n], 4) for n in ns}
                if "G_1" in med:
                    rec["joint"]["J_over_G"] = {n: round(med["J_%d" % n] / med["G_%d" % n], 4) for n in ns}
            if a.envelope:
                E = med["E_traj"] + med["E_reduce"]
                rec["envelope"] = dict(E_ms=round(E, 4), B_env_over_E=round(med["B_env"] / E, 4),
                                       B_env_over_B_stats=round(med["B_env"] / med["B_stats"], 4))
            if a.histogram:
                Q = med["Q_traj"] + min(med["Q_count"], med["Q_sort"])
                spread = lambda k: round((max(ms[k]) - min(ms[k])) / med[k], 4)
                rec["histogram"] = dict(H_ms=med["H"], C_ms=med["B_stats"], E_ms=med["B_env"], Q_ms=round(Q, 4),
                                        H_over_C=round(med["H"] / med["B_stats"], 4), H_over_E=round(med["H"] / med["B_env"], 4),
                                        H_over_Q=round(med["H"] / Q, 4), H_one_bin_over_H=round(med["H_one_bin"] / med["H"], 4),
                                        spread_rel=dict(H=spread("H"), C=spread("B_stats"), E=spread("B_env")))
                if a.hist_valu:
                    roof = (B / 64) * (a.T - 1) * a.hist_valu * CYCLES_PER_VALU / (SIMDS * CLOCK_HZ) * 1e3
                    rec["histogram"]["vector_issue"] = dict(valu_per_stage=a.hist_valu, roof_ms=round(roof, 4),
                                                            share_H=round(roof / med["H"], 3))
            stages = B * (a.T - 1)
            rec["member_stages_per_s"] = {k: round(stages / (med[k] * 1e-3), 0) for k in ms}
            if a.valu:
                roof_ms = (B / 64) * (a.T - 1) * a.valu * CYCLES_PER_VALU / (SIMDS * CLOCK_HZ) * 1e3
                rec["vector_issue"] = dict(valu_per_stage=a.valu, roof_ms=round(roof_ms, 4),
                                           share_B_stats=round(roof_ms / med["B_stats"], 3), bound="issue")
        out["sizes"].append(rec)
        del runs
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
