"""aoc_track_ensemble_lqg_limited / batch.track_ensemble(filter=, u_min= / u_max= / u_rate=, est_input=): noisy measurements,
a Kalman estimate and a saturating actuator in one loop.

Two bars.  The limits and the estimator's correction are selections, so with infinite limits every output is
aoc_track_ensemble_lqg's bit for bit.  With finite limits the checker is lqg_loop_limited of tests/test_lqg_limits_abi.py,
and the bar is the one of tests/test_gpu_lqg.py: 16 times the checker's own rounding (REF_GAP_LIM, fp64 against
np.longdouble, measured there on exactly these cases) under scaled_gap — and the cut statistics EXACTLY, which the
conditions asserted there allow: no demand of a checked member comes near a bound."""
import numpy as np
import pytest

from test_gpu_covariance import MC_SEED, MC_T, g4_jacobians, mc_members
from test_gpu_ensemble import DELTA_SCALE, SIGMA, _g4, _problem
from test_gpu_lqg import (CASES, GEOMETRY, KEYS, RHO, SEED, ST_NAN, ST_VNONPOS, case_inputs, mc_z, scaled_gap, selection,
                          setup)
from test_limits_abi import INF2, U_MAX, U_MIN, U_RATE
from test_lqg_limits_abi import (EDGE_B, EDGE_T, EST_INPUTS, ISO_HI, ISO_LO, ISO_RATE, MC_HI, MC_LO, MC_RATE, PARITY_B,
                                 PARITY_T, REF_GAP_LIM, checker_limited, limits_for, sat_of)

pytestmark = pytest.mark.gpu

TOL = 16 * REF_GAP_LIM
NONE = dict(u_min=-INF2, u_max=INF2, u_rate=INF2)
LIM_KEYS = KEYS + ("sat",)


def _lim(lims):
    return dict(u_min=lims[0], u_max=lims[1], u_rate=lims[2])


def _run(XO, UO, KK, L, d, mpo, sigma=None, rho=None, e0=None, trajectories=True, weights=None, **kw):
    from aircraftoptimalcontrol_amd import batch
    g = g4_jacobians()[0]
    bp = _problem(dict(g, xx_opt=XO[0]), weights)
    return batch.track_ensemble(bp, XO, UO, delta=d, KK=KK, members_per_opt=mpo, sigma=sigma, seed=SEED, filter=L, rho=rho,
                                ehat0=e0, trajectories=trajectories, **kw)


def _same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    if "sat_count" in a and "sat_count" in b:
        assert np.array_equal(np.stack(a["sat_count"]), np.stack(b["sat_count"])), (what, "sat_count")


def _never_cut(r, T, B, n_opt):
    assert r["sat"].shape == (B, 6) and not r["sat"][:, 0:2].any() and (r["sat"][:, 2:4] == T).all()
    assert not r["sat"][:, 4:6].any() and not np.signbit(r["sat"][:, 4:6]).any()
    assert len(r["sat_count"]) == n_opt
    for c in r["sat_count"]:
        assert c.shape == (T, 2) and c.dtype == np.int32 and not c.any()
    assert all(np.array_equal(sm["frac_cut"], [0.0, 0.0]) for sm in r["summary"])


@pytest.mark.parametrize("B", [65, 130])
@pytest.mark.parametrize("T", [3, 17, 33])
def test_infinite_limits_change_no_bit(T, B):
    """lo = -inf, hi = +inf, rate = +inf, both values of est_input, all six cases, with trajectories and without: every key
    of KEYS has the bits of aoc_track_ensemble_lqg, sat reads "never cut" and sat_count is all zero."""
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    for name in CASES:
        sigma, rho, e0 = case_inputs(name, T, B, n_opt)
        old = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0)
        old_so = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, trajectories=False)
        assert "sat" not in old and "est_input" not in old
        for est_input in EST_INPUTS:
            r = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, est_input=est_input, **NONE)
            _same(r, old, KEYS, (name, est_input))
            _never_cut(r, T, B, n_opt)
            assert r["est_input"] == est_input
            so = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, trajectories=False, est_input=est_input, **NONE)
            _same(so, old_so, ("stats", "est_stats", "status"), (name, est_input, "statistics only"))
            _never_cut(so, T, B, n_opt)


def test_infinite_limits_with_float32_storage_and_dense_weights():
    """the two float32-state instances (ehat0, no noise: the only form float32 storage takes) and the dense-weight ones,
    130 members, T = 33: the bits of aoc_track_ensemble_lqg; with sigma or rho float32 storage is refused as there"""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_dense import _tracking_weights
    T, B = 33, 130
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    sigma, rho, e0 = case_inputs("ehat0", T, B, n_opt)
    for w in (None, _tracking_weights()):
        for f32 in (False, True):
            sg, rh = (None, None) if f32 else (sigma, rho)
            old = _run(XO, UO, KK, L, d, mpo, sg, rh, e0, weights=w, f32=f32)
            for est_input in EST_INPUTS:
                r = _run(XO, UO, KK, L, d, mpo, sg, rh, e0, weights=w, f32=f32, est_input=est_input, **NONE)
                _same(r, old, KEYS, (w is None, f32, est_input))
                _never_cut(r, T, B, n_opt)
    with pytest.raises(batch.AocError, match="float32 state storage .* cannot hold disturbed states"):
        _run(XO, UO, KK, L, d, mpo, SIGMA, RHO, e0, f32=True, est_input="applied", **NONE)


def _parity(T, B):
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    sel, lims = selection(B), limits_for(T, B)
    for name in CASES:
        sigma, rho, e0 = case_inputs(name, T, B, n_opt)
        for est_input in EST_INPUTS:
            r = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, est_input=est_input, **_lim(lims))
            assert r["xx_reg"].shape == (B, 6, T) and r["sat"].shape == (B, 6) and not r["status"].any()
            xx, uu, xh, es, vv, cut = checker_limited(mdl, XO, UO, KK, L, jac, d, mpo, sel, e0,
                                                      r["dist"] if sigma is not None else None,
                                                      r["meas"] if rho is not None else None, lims, est_input)
            assert cut[:, 0].any() and cut[:, 1].any(), (T, B, name, est_input)
            worst = 0.0
            for i, m in enumerate(sel):
                k = m // mpo
                got = (r["xx_reg"][m:m + 1], r["uu_reg"][m:m + 1], r["xhat"][m:m + 1], r["est_stats"][m:m + 1])
                worst = max(worst, scaled_gap(got, [v[i:i + 1] for v in (xx, uu, xh, es)], XO[k], UO[k]))
            print("T = %d, B = %d, %s, %s: scaled gap %.3g (bound %.3g)" % (T, B, name, est_input, worst, TOL))
            assert worst <= TOL, (T, B, name, est_input, worst)
            want = sat_of(vv, uu, cut)
            assert np.array_equal(r["sat"][sel, 0:4], want[:, 0:4]), (T, B, name, est_input)
            scale = np.stack([np.abs(uu[i] - UO[m // mpo])[:, :T - 1].max(axis=1) for i, m in enumerate(sel)])
            assert (np.abs(r["sat"][sel, 4:6] - want[:, 4:6]) <= TOL * scale).all(), (T, B, name, est_input)
    return r


@pytest.mark.parametrize("B", PARITY_B)
@pytest.mark.parametrize("T", PARITY_T)
def test_parity_with_the_checker(T, B):
    """The sizes and cases of tests/test_gpu_lqg.py under the limits limits_for(T, B), both values of est_input, the checker
    fed the device's own dist and meas: xx, uu, xhat and est_stats within 16 x REF_GAP_LIM under scaled_gap; the number of cut
    samples and the first cut sample exactly; max |v - u| within the same tolerance of the input's scale.  Both channels are
    cut among the checked members in every case (asserted)."""
    _parity(T, B)


@pytest.mark.parametrize("T", EDGE_T)
def test_parity_at_the_horizon_edges(T):
    """the same at the horizons on both sides of the estimator's block reload, 65 members"""
    _parity(T, EDGE_B)


def test_sat_count_is_the_count_over_the_cut_flags():
    """B = 64, T = 17, noise + rho + ehat0: sat_count equals NumPy's count over the checker's cut flags of all 64 members,
    sample T-1 is zero.  B = 130 about three optima: sat_count summed over the samples equals the members' sat[0..1] summed
    over each optimum's members (all stay in the domain); the same counts without trajectories."""
    T = 17
    for est_input in EST_INPUTS:
        XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, 64)
        sigma, rho, e0 = case_inputs("ehat0", T, 64, n_opt)
        lims = limits_for(T, 64)
        r = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, est_input=est_input, **_lim(lims))
        cut = checker_limited(mdl, XO, UO, KK, L, jac, d, mpo, np.arange(64), e0, r["dist"], r["meas"], lims, est_input)[5]
        assert (r["first_bad"] == T).all() and cut[:, 0].any() and cut[:, 1].any()
        assert r["sat_count"][0].dtype == np.int32 and np.array_equal(r["sat_count"][0], cut.sum(axis=0).T)
        assert not r["sat_count"][0][T - 1].any()
        assert np.array_equal(r["summary"][0]["frac_cut"], cut.any(axis=2).mean(axis=0))
        XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, 130)
        sigma, rho, e0 = case_inputs("ehat0", T, 130, n_opt)
        r = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, est_input=est_input, **_lim(limits_for(T, 130)))
        so = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, trajectories=False, est_input=est_input, **_lim(limits_for(T, 130)))
        assert (r["first_bad"] == T).all() and r["sat"][:, 0:2].any()
        for k in range(n_opt):
            members = slice(k * mpo, min((k + 1) * mpo, 130))
            assert np.array_equal(r["sat_count"][k].sum(axis=0), r["sat"][members, 0:2].sum(axis=0)), (est_input, k)
            assert np.array_equal(so["sat_count"][k], r["sat_count"][k])
        assert r["sat_count"][2].max() <= 2                                # the third optimum has two members


def test_the_correction_stays_in_its_lane():
    """Moment-only limits (ISO_LO / ISO_HI), 64 members, T = 200, noise + rho: the members that are never cut have identical
    bits in every output under "applied" and "demanded" — and those of aoc_track_ensemble_lqg —, at least 8 of each kind
    exist, thrust is never cut, and at least one cut member's xhat differs between the two."""
    T, B = 200, 64
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    lim = dict(u_min=ISO_LO, u_max=ISO_HI, u_rate=ISO_RATE)
    a = _run(XO, UO, KK, L, d, mpo, SIGMA, RHO, est_input="applied", **lim)
    b = _run(XO, UO, KK, L, d, mpo, SIGMA, RHO, est_input="demanded", **lim)
    old = _run(XO, UO, KK, L, d, mpo, SIGMA, RHO)
    free = (a["sat"][:, 1] == 0) & (b["sat"][:, 1] == 0)
    hit = (a["sat"][:, 1] > 0) & (b["sat"][:, 1] > 0)
    assert free.sum() >= 8 and hit.sum() >= 8 and not a["sat"][:, 0].any() and not b["sat"][:, 0].any()
    for k in LIM_KEYS:
        assert np.array_equal(a[k][free], b[k][free]), k
    for k in KEYS:
        assert np.array_equal(a[k][free], old[k][free]), k
    assert any(not np.array_equal(a["xhat"][m], b["xhat"][m]) for m in np.flatnonzero(hit))
    assert not np.array_equal(a["est_stats"][hit], b["est_stats"][hit])


def test_bits_do_not_depend_on_the_cut_the_tile_the_outputs_or_the_run():
    """130 members about three optima, noise + rho + ehat0, T = 33, the fixed limits, est_input = applied: the same call
    again gives the same bits; without trajectories the statistics, sat and sat_count are the same; cut into two calls with
    first= (members 0-63, 64-129) it gives the bits of one call and sat_count_merge is not needed across optima; the third
    optimum's members run alone (tile 0) have the bits they had as tile 2 of 3; and sat_count = NULL at the C ABI changes
    no other output."""
    import ctypes as C
    import torch
    from aircraftoptimalcontrol_amd import _lib, batch
    T, B = 33, 130
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    sigma, rho, e0 = case_inputs("ehat0", T, B, n_opt)
    kw = dict(est_input="applied", **_lim((U_MIN, U_MAX, U_RATE)))
    r = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, **kw)
    assert r["sat"][:, 0].any() and r["sat"][:, 1].any()
    _same(r, _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, **kw), LIM_KEYS, "again")
    so = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, trajectories=False, **kw)
    assert "xhat" not in so and "xx_reg" not in so
    _same(r, so, ("stats", "est_stats", "status", "sat"), "statistics only")
    a = _run(XO[:1], UO[:1], KK[:1], L[:1], d[:64], mpo, sigma, rho, e0[:1], first=0, **kw)
    b = _run(XO[1:], UO[1:], KK[1:], L[1:], d[64:], mpo, sigma, rho, e0[1:], first=64, **kw)
    for k in LIM_KEYS:
        assert np.array_equal(np.concatenate([a[k], b[k]]), r[k]), k
    assert np.array_equal(np.stack(a["sat_count"] + b["sat_count"]), np.stack(r["sat_count"]))
    c = _run(XO[2:], UO[2:], KK[2:], L[2:], d[128:], mpo, sigma, rho, e0[2:], first=128, **kw)
    for k in LIM_KEYS:
        assert np.array_equal(c[k], r[k][128:]), k
    assert np.array_equal(c["sat_count"][0], r["sat_count"][2])
    # the C ABI with sat_count = NULL and statistics only
    bp = _problem(dict(g4_jacobians()[0], xx_opt=XO[0]))
    dev, ptr = bp.device, batch._ptr
    grp = np.arange(B) // mpo
    nominal = torch.from_numpy(batch.ensemble_nominal(XO, UO, KK)).to(dev)
    filt, x0t = batch._filter_to_device(L, n_opt, T, dev), batch.pack_vec(XO[grp, :, 0] + d, dev)
    e0_d = batch._dev_f64(np.ascontiguousarray(e0), dev)
    nz = _lib.MpcNoise(SEED, 0, 0, (C.c_double * 6)(*sigma.tolist()))
    rho_c = (C.c_double * 6)(*rho.tolist())
    lim = _lib.ActuatorLimits((C.c_double * 2)(*U_MIN.tolist()), (C.c_double * 2)(*U_MAX.tolist()), (C.c_double * 2)(*U_RATE.tolist()))
    nt = batch.ntiles(B)
    stats = torch.empty((nt, _lib.AOC_ENS_NSTAT, batch.TILE), dtype=torch.float64, device=dev)
    est_stats = torch.empty((nt, _lib.AOC_LQG_NSTAT, batch.TILE), dtype=torch.float64, device=dev)
    sat = torch.empty((nt, _lib.AOC_SAT_NSTAT, batch.TILE), dtype=torch.float64, device=dev)
    status = torch.zeros(nt * batch.TILE, dtype=torch.int32, device=dev)
    nbytes = int(_lib.lib().aoc_track_ensemble_lqg_limited_scratch_bytes(B, n_opt, T, mpo, 0))
    assert nbytes == int(_lib.lib().aoc_track_ensemble_lqg_scratch_bytes(n_opt, T))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    p = bp.c_problem(B)
    _lib.check(_lib.lib().aoc_track_ensemble_lqg_limited(C.byref(p), n_opt, mpo, ptr(nominal), ptr(filt), ptr(x0t), ptr(e0_d),
                                                         C.byref(nz), rho_c, C.byref(lim), _lib.EST_INPUT_APPLIED, None, None,
                                                         None, None, None, ptr(stats), ptr(est_stats), ptr(sat), None,
                                                         ptr(status), ptr(scratch), nbytes), "aoc_track_ensemble_lqg_limited")
    assert np.array_equal(batch.unpack_vec(stats, B).cpu().numpy(), r["stats"])
    assert np.array_equal(batch.unpack_vec(est_stats, B).cpu().numpy(), r["est_stats"])
    assert np.array_equal(batch.unpack_vec(sat, B).cpu().numpy(), r["sat"])
    assert np.array_equal(status[:B].cpu().numpy(), r["status"])


def test_a_bad_member_among_good_ones():
    """The two bad members of tests/test_gpu_lqg.py (V_0 = -24; a NaN component) among 62 ordinary ones, noise + rho, the
    fixed limits, both values of est_input: both are flagged with first_bad = 0, the others keep every bit, sat_count is the
    count over the others alone, the NaN sticks in the error statistics, and the NaN member's demand stays NaN and is never
    counted as cut."""
    T = 33
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, 64)
    d2 = d.copy()
    d2[17] = [0, 0, -40, 0, 0, 0]
    d2[40, 4] = np.nan
    assert XO[0, 2, 0] - 40 < 0
    others = np.setdiff1d(np.arange(64), [17, 40])
    for est_input in EST_INPUTS:
        kw = dict(est_input=est_input, **_lim((U_MIN, U_MAX, U_RATE)))
        clean = _run(XO, UO, KK, L, d, mpo, SIGMA, RHO, **kw)
        r = _run(XO, UO, KK, L, d2, mpo, SIGMA, RHO, **kw)
        assert (clean["first_bad"] == T).all() and not clean["status"].any() and clean["sat_count"][0].any()
        assert r["status"][17] & ST_VNONPOS and r["first_bad"][17] == 0
        assert r["status"][40] & ST_NAN and r["first_bad"][40] == 0
        for k in LIM_KEYS:
            assert np.array_equal(r[k][others], clean[k][others]), (est_input, k)
        assert np.isnan(r["max_e"][40]).any() and np.isnan(r["sum_e2"][40]).any()
        # the counts: every member of `clean` counts at every sample, members 17 and 40 of `r` at none
        cut = checker_limited(mdl, XO, UO, KK, L, jac, d, mpo, np.arange(64), None, clean["dist"], clean["meas"],
                              (U_MIN, U_MAX, U_RATE), est_input)[5]
        assert np.array_equal(clean["sat_count"][0], cut.sum(axis=0).T)
        assert np.array_equal(r["sat_count"][0], cut[others].sum(axis=0).T)
        assert np.isnan(r["uu_reg"][40, :, :T - 1]).all()               # a NaN demand stays NaN ...
        assert not r["sat"][40, 0:2].any() and (r["sat"][40, 2:4] == T).all() and np.isnan(r["sat"][40, 4:6]).all()   # ... uncut
        assert r["summary"][0]["n_bad"] == 2


@pytest.mark.parametrize("est_input", EST_INPUTS)
def test_estimation_error_under_limits_against_the_filters_own_covariance(est_input):
    """2048 members, T = 200, s = 0.1, SIGMA, RHO, the device's own Kalman gains (filter="device") and the limits MC_LO /
    MC_HI / MC_RATE, which cut every member: the error of the estimator that is told the applied input agrees with the
    filter's own P^+ within sampling error (both z <= 5), the one left with its demand does not (z_cov >= 15) — the bounds
    the CPU checker meets alone (tests/test_lqg_limits_abi.py)."""
    from aircraftoptimalcontrol_amd import batch
    g = _g4()[0]
    T = MC_T
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    d, _, S0 = mc_members(0.1)
    bp = _problem(dict(g, xx_opt=xo))
    P_post = batch.filter_gains_device(bp, xo, uo, S0, SIGMA, RHO)[2][0]
    r = batch.track_ensemble(bp, xo, uo, delta=d, KK=KK, sigma=SIGMA, seed=MC_SEED, filter="device", Sigma0=S0, rho=RHO,
                             trajectories=True, u_min=MC_LO, u_max=MC_HI, u_rate=MC_RATE, est_input=est_input)
    assert not r["status"].any() and not r["filter_status"].any() and (r["first_bad"] == T).all()
    err = (r["xx_reg"] - xo[None]) - (r["xhat"] - xo[None])
    zc, zm = mc_z(err, P_post)
    frac = r["summary"][0]["frac_cut"]
    print("%s: z_cov = %.3g, z_mean = %.3g, frac_cut %s" % (est_input, zc, zm, frac))
    assert frac[0] > 0.9 and frac[1] > 0.5
    u = r["uu_reg"][:, :, :T - 1]
    assert ((u >= MC_LO[None, :, None]) & (u <= MC_HI[None, :, None])).all()
    if est_input == "applied":
        assert zc <= 5 and zm <= 5, (zc, zm)
    else:
        assert zc >= 15, zc


def test_example_prints_frac_cut_and_the_estimation_error(tmp_path):
    """examples/run_tracking_ensemble.py --rho --u-min --u-max --u-rate --est-input applied as a process: one JSON line with
    est_input, frac_cut and the RMS estimation error of batch.track_ensemble for the same seeded members."""
    import json
    from test_gpu_drivers import _run as run_example
    from aircraftoptimalcontrol_amd import batch, problems
    g = _g4()[0]
    T = 200
    xo, uo = g["xx_opt"][:, :T], g["uu_opt"][:, :T]
    np.save(tmp_path / "xx_star.npy", xo)
    np.save(tmp_path / "uu_star.npy", uo)
    out = run_example("run_tracking_ensemble.py", "--data", tmp_path, "--members", 256, "--seed", 5, "--dt", float(g["dt"]),
                      "--sigma", *SIGMA, "--rho", *RHO, "--u-min", *U_MIN, "--u-max", *U_MAX, "--u-rate", *U_RATE,
                      "--est-input", "applied")
    line = json.loads(out.strip().split("\n")[-1])
    assert line["members"] == 256 and line["T"] == T and line["est_input"] == "applied"
    assert line["limits"] == dict(u_min=U_MIN.tolist(), u_max=U_MAX.tolist(), u_rate=U_RATE.tolist())
    Q, R, QT = problems.tracking_weights()
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]))
    L = batch.filter_gains(bp, xo, uo, np.diag(DELTA_SCALE ** 2), SIGMA, RHO)[0]
    d = np.random.default_rng(5).normal(size=(256, 6)) * DELTA_SCALE
    r = batch.track_ensemble(bp, xo, uo, delta=d, sigma=SIGMA, seed=5, filter=L, rho=RHO, u_min=U_MIN, u_max=U_MAX,
                             u_rate=U_RATE, est_input="applied")
    assert np.array_equal(np.asarray(line["frac_cut"]), r["summary"][0]["frac_cut"]) and r["summary"][0]["frac_cut"][0] > 0
    assert np.array_equal(np.asarray(line["rms_estimation_error"]), np.sqrt(r["sum_e2"].mean(axis=0) / T))
    assert line["left_the_domain"] == r["summary"][0]["n_bad"]
