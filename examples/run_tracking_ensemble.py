#!/usr/bin/env python3
"""Closed-loop tracking ensemble about a saved optimum (the robustness sample of lqr_tracking.py:245-283, many times over):
loads Data/xx_star.npy, Data/uu_star.npy (what run_newton.py writes), computes the tracking gains once, rolls out
--members perturbed and disturbed closed loops on the device and prints the distribution of the tracking errors as one
JSON line.

    python examples/run_tracking_ensemble.py [--data Data] [--members 65536] [--sigma 1e-3 1e-3 1e-2 1e-4 1e-3 1e-4]
                                             [--delta 0.3 0.3 0.5 0.05 0.1 0.05] [--seed 1] [--dt 1e-3]
                                             [--envelope FILE.npz] [--quantiles FILE.npz [--q 0.05 0.5 0.95]]
                                             [--predict FILE.npz] [--rho r0 r1 r2 r3 r4 r5 [--device-gains] [--measured c ...]
                                                                   [--predict-joint FILE.npz]]
                                             [--u-min a b] [--u-max a b] [--u-rate a b] [--est-input applied|demanded]

--envelope FILE.npz: also reduce over the members at every sample on the device (the tube around the optimum) and save
n (T,), min_dx / max_dx (6,T), min_du / max_du (2,T), mean_dx (6,T), cov_dx (6,6,T), raw (T,44); the JSON line then
carries "envelope": the file, n at the last sample and the largest band width max_dx - min_dx per state.
--quantiles FILE.npz: also the quantile tubes --q over the members at every sample, from a 64-bin histogram counted on the
device in a second pass over the same members (bins from the min / max of the first), and save quantiles (len(q),), n (T,),
hist (T,8,64), bins (T,8,2) = (lo, inv_w), tube (len(q),8,T), tube_width (8,T) (channels dx[0..5], du[0..1]); the JSON
line then carries "quantiles": the file, q and the largest width of the tube (last level - first level) per state.
--predict FILE.npz: also what linear theory predicts for the same loop (the Lyapunov recursion about the optimum with the
tracking gains, from the population moments of the initial perturbation, --delta, and --sigma) and save mean_dx (6,T),
cov_dx (6,6,T), mean_du (2,T), cov_du (2,2,T), raw (T,32): the tube the sampled one of --envelope is read against; the JSON
line then carries "predict": the file and the largest predicted standard deviation per state.
--rho r0 .. r5: no member feeds back its true state but a Kalman estimate from measurements of the deviation with noise of
these standard deviations (batch.filter_gains about the optimum, prior spread --delta, --sigma; aoc_track_ensemble_lqg); the
JSON line then carries "rho" and "rms_estimation_error", per channel the root of the mean over members and samples of the
squared estimation error.  Not together with --envelope, --quantiles or --predict.
--device-gains (takes effect only with --rho): the filter's gains are computed on the device (aoc_filter_gains) and handed to
the ensemble as they lie, batch.track_ensemble(filter="device"); --measured c ...: the filter then measures these channels
only (default: all six).  The JSON line then also carries "device_gains": true and "measured".
--predict-joint FILE.npz (with --rho): also what linear theory predicts for THIS loop (aoc_track_covariance_lqg with the same
gains, from the population moments of the initial perturbation, --sigma and --rho) and save mean_dx, mean_e (6,T), cov_dx,
cov_e, cov_dx_e, cov_xhat (6,6,T), mean_du (2,T), cov_du (2,2,T), raw (T,96), status; the JSON line then carries
"predict_joint": the file, and "predicted_rms_dx" / "predicted_rms_estimation_error" beside the sampled "rms_dx" /
"rms_estimation_error": per channel the root of the mean over the samples of variance + mean^2.  The members' trajectories
are then kept on the device to sample rms_dx (26 doubles per member and sample).
--u-min a b, --u-max a b, --u-rate a b (thrust, pitching moment; any of the three, inf = unbounded): the demand of every
member is cut to the range and, from sample 1 on, to within u-rate * dt of the input before (aoc_track_ensemble_limited);
every other output is then that of the limited loop (--predict stays the prediction of the UNLIMITED linear loop).  The JSON
line then carries "limits": the three pairs (null = unbounded), and "frac_cut": per channel the share of members cut at
least once.  Together with --rho they need --est-input.
--est-input applied | demanded (with --rho and a limit; aoc_track_ensemble_lqg_limited): the demand formed from the estimate is
cut, and the estimator's prediction is told the applied input ("applied": it adds B_t (u_t - v_t) where a sample is cut) or
left with its demand ("demanded": the estimator of --rho as it is, which a cut misleads).  The JSON line then carries
"est_input" beside "limits", "frac_cut", "rho" and "rms_estimation_error".  --predict-joint stays the prediction of the loop
WITHOUT limits.
"""
import argparse
import json
import os

import numpy as np

import _common  # noqa: F401
from aircraftoptimalcontrol_amd import batch, problems


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="Data")
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--sigma", type=float, nargs=6, default=None, help="std of the state disturbance per step (default: none)")
    ap.add_argument("--delta", type=float, nargs=6, default=[0.3, 0.3, 0.5, 0.05, 0.1, 0.05],
                    help="std of the perturbation of the initial state")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--envelope", default=None, metavar="FILE.npz", help="save the per-sample envelope over the members")
    ap.add_argument("--quantiles", default=None, metavar="FILE.npz", help="save per-sample quantile tubes over the members")
    ap.add_argument("--predict", default=None, metavar="FILE.npz", help="save the linear prediction of mean and covariance")
    ap.add_argument("--rho", type=float, nargs=6, default=None, help="std of the measurement noise: a Kalman estimate in the loop")
    ap.add_argument("--device-gains", action="store_true", help="with --rho: the filter's gains from aoc_filter_gains")
    ap.add_argument("--measured", type=int, nargs="+", default=None, help="with --device-gains: the channels the filter measures")
    ap.add_argument("--predict-joint", default=None, metavar="FILE.npz",
                    help="with --rho: save the joint linear prediction of dx and of the estimation error")
    ap.add_argument("--u-min", type=float, nargs=2, default=None, metavar=("THRUST", "MOMENT"), help="lower limit of the inputs")
    ap.add_argument("--u-max", type=float, nargs=2, default=None, metavar=("THRUST", "MOMENT"), help="upper limit of the inputs")
    ap.add_argument("--u-rate", type=float, nargs=2, default=None, metavar=("THRUST", "MOMENT"),
                    help="largest change of the inputs per second")
    ap.add_argument("--est-input", choices=("applied", "demanded"), default=None,
                    help="with --rho and a limit: what the estimator's prediction is told")
    ap.add_argument("--q", type=float, nargs="+", default=[0.05, 0.5, 0.95], help="quantile levels of --quantiles")
    a = ap.parse_args()
    if a.rho is not None and (a.envelope or a.quantiles or a.predict):
        ap.error("--rho does not combine with --envelope, --quantiles or --predict")
    limits = {k: v for k, v in (("u_min", a.u_min), ("u_max", a.u_max), ("u_rate", a.u_rate)) if v is not None}
    if limits and a.rho is not None and a.est_input is None:
        ap.error("--u-min / --u-max / --u-rate combine with --rho only with --est-input applied | demanded (what the "
                 "estimator's prediction is told once the input is cut)")
    if a.est_input is not None and not (limits and a.rho is not None):
        ap.error("--est-input goes with --rho and a limit (--u-min / --u-max / --u-rate)")
    lqg_limits = dict(est_input=a.est_input, **limits) if a.est_input is not None else {}
    if a.predict_joint is not None and a.rho is None:
        ap.error("--predict-joint goes with --rho (the prediction of the loop with the estimator; --predict is the other one)")
    xx_opt = np.load(os.path.join(a.data, "xx_star.npy"))
    uu_opt = np.load(os.path.join(a.data, "uu_star.npy"))
    T = xx_opt.shape[1]
    Q, R, QT = problems.tracking_weights()                           # lqr_tracking.py:324-328
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), a.dt)
    delta = np.random.default_rng(a.seed).normal(size=(a.members, 6)) * np.asarray(a.delta)
    device_gains = a.rho is not None and a.device_gains
    joint = dict(predict_joint=True, mean0=np.zeros(6), trajectories=True, to_host=False) if a.predict_joint is not None else {}
    if device_gains:
        r = batch.track_ensemble(bp, xx_opt, uu_opt, delta=delta, sigma=a.sigma, seed=a.seed, filter="device", rho=a.rho,
                                 Sigma0=np.diag(np.asarray(a.delta) ** 2), measured=a.measured, **joint, **lqg_limits)
    elif a.rho is not None:
        L = batch.filter_gains(bp, xx_opt, uu_opt, np.diag(np.asarray(a.delta) ** 2), a.sigma, a.rho)[0]
        r = batch.track_ensemble(bp, xx_opt, uu_opt, delta=delta, sigma=a.sigma, seed=a.seed, filter=L, rho=a.rho,
                                 Sigma0=np.diag(np.asarray(a.delta) ** 2) if joint else None, **joint, **lqg_limits)
    else:
        r = batch.track_ensemble(bp, xx_opt, uu_opt, delta=delta, sigma=a.sigma, seed=a.seed, envelope=a.envelope is not None,
                                 quantiles=a.q if a.quantiles is not None else None, predict=a.predict is not None,
                                 mean0=np.zeros(6), Sigma0=np.diag(np.asarray(a.delta) ** 2), **limits)
    sm = r["summary"][0]
    tolist = lambda d: {k: np.asarray(v).tolist() for k, v in d.items()}
    line = dict(members=a.members, T=T, sigma=a.sigma, left_the_domain=sm["n_bad"],
                max_dx=tolist(sm["max_dx"]), final_dx=tolist(sm["final_dx"]), cost=tolist(sm["cost"]))
    if limits:
        finite = lambda v: [float(c) if np.isfinite(c) else None for c in v]
        line.update(limits={k: finite(v) for k, v in r["limits"].items()}, frac_cut=sm["frac_cut"].tolist())
    if a.rho is not None:
        line.update(rho=list(a.rho), rms_estimation_error=np.sqrt(r["sum_e2"].mean(axis=0) / T).tolist())
    if a.est_input is not None:
        line.update(est_input=r["est_input"])
    if a.predict_joint is not None:
        pj = r["predicted_joint"][0]
        np.savez(a.predict_joint, status=r["predicted_joint_status"][0], **pj)
        import torch
        dx = r["xx_reg"] - torch.from_numpy(xx_opt).to(r["xx_reg"].device)[None]
        rms = lambda mean, cov: np.sqrt((np.einsum("iit->it", cov) + mean ** 2).mean(axis=1)).tolist()
        line.update(predict_joint=a.predict_joint, rms_dx=torch.sqrt((dx * dx).mean(dim=(0, 2))).cpu().numpy().tolist(),
                    predicted_rms_dx=rms(pj["mean_dx"], pj["cov_dx"]),
                    predicted_rms_estimation_error=rms(pj["mean_e"], pj["cov_e"]))
    if device_gains:
        line.update(device_gains=True, measured=sorted(set(a.measured)) if a.measured is not None else list(range(6)))
    if a.envelope is not None:
        env = r["envelope"][0]
        np.savez(a.envelope, **env)
        some = env["n"] > 0                                          # an empty sample has the band +inf .. -inf
        width = (env["max_dx"] - env["min_dx"])[:, some]
        line["envelope"] = dict(file=a.envelope, n_last=int(env["n"][-1]),
                                max_width=width.max(axis=1).tolist() if some.any() else None)
    if a.quantiles is not None:
        tube = r["tube"][0]
        np.savez(a.quantiles, quantiles=np.asarray(r["quantiles"]), n=r["envelope"][0]["n"], hist=r["hist"][0], bins=r["bins"][0],
                 tube=tube, tube_width=r["tube_width"][0])
        with np.errstate(all="ignore"):
            span = tube[-1, :6] - tube[0, :6]                        # NaN where no member counts
        line["quantiles"] = dict(file=a.quantiles, q=list(r["quantiles"]),
                                 max_tube_width=np.nanmax(span, axis=1).tolist() if np.isfinite(span).any() else None)
    if a.predict is not None:
        pred = r["predicted"][0]
        np.savez(a.predict, **pred)
        std = np.sqrt(np.einsum("iit->it", pred["cov_dx"]))
        line["predict"] = dict(file=a.predict, max_std=std.max(axis=1).tolist())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
