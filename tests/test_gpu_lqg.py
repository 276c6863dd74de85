"""aoc_track_ensemble_lqg / batch.track_ensemble(filter=, rho=, ehat0=): noisy measurements and a Kalman estimate in the loop.

The checker is lqg_loop below: the loop of include/aoc.h in NumPy, the plant through the oracle's Dynamics.step, the input
summed as tests/test_gpu_ensemble.py host_loop sums it, F_t and c_t from the oracle's Jacobians (tests/test_lqg_abi.py checks
it without a GPU).  The device differs from it in fused multiply-adds and in the Jacobians' own sin / cos, so the bar is not
bit-identity but a multiple of the checker's OWN rounding: the largest scaled gap between the checker in fp64 and the same
checker with the estimate, L nu and F e in np.longdouble (the plant in fp64 both times) over the cases of the parity tests
(REF_GAP, measured on the CPU by reference_gap below), times 16 — the margin of tests/test_gpu_covariance.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_covariance import MC_M, MC_SEED, MC_T, g4_jacobians, mc_members, offset_nominal, windows, z_scores  # noqa: F401
from test_gpu_ensemble import DELTA_SCALE, SIGMA, _g4, _problem, deltas, numpy_stats

pytestmark = pytest.mark.gpu

ST_NAN, ST_VNONPOS = 1, 2
RHO = 0.1 * DELTA_SCALE
SEED = 20261019
# the largest scaled gap (metric: scaled_gap below) between lqg_loop in fp64 and with the estimator in np.longdouble over
# every case of test_parity_with_the_checker and test_a_nominal_that_is_not_a_rollout, measured: 4.12e-14 (T = 200 with the
# disturbance alone; the states of the two checkers agree bit for bit, so no float32 rounding of the plant flipped between
# them); the device may be 16x that
REF_GAP = 4.2e-14
TOL = 16 * REF_GAP
SIZES_T = (3, 17, 33, 200)
# The horizon edges, run for B = 65 alone: a block of F / c / L records is reloaded while b * 16 <= T - 1, so at T = 16 and
# 32 sample T-1 is the last record of a block and the next block is never loaded, at T = 18 the second block holds one
# stage, and T = 4 is the first horizon with a stage that is neither the first nor the last.
EDGE_T = (4, 16, 18, 32)
EDGE_B = 65
GEOMETRY = {1: (1, 64), 64: (1, 64), 65: (1, 128), 130: (3, 64)}   # members -> (n_opt, members_per_opt)
# case -> (disturbance, measurement noise: True = RHO, "zero" = a rho of six zeros, False = rho NULL; ehat0)
CASES = {"plain": (False, False, False), "noise": (True, False, False), "noise_rho": (True, True, False),
         "ehat0": (True, True, True), "rho_only": (False, True, False), "rho_zero": (True, "zero", False)}


def lqg_loop(mdl, xo, uo, KK, L, jac, x0, ehat0=None, dist=None, meas=None, dtype=np.float64):
    """The loop of aoc_track_ensemble_lqg for M members about ONE optimum: xo (6,T), uo (2,T), KK (2,6,T), L (6,6,T), jac =
    jacobians(mdl, xo, uo), x0 (M,6), ehat0 (6,) or None, dist / meas (M,6,T) or None = what is added to form sample t+1 /
    the measurement noise v_t.  The estimate, L nu and F e are computed in `dtype`, the plant and the input in fp64.
    -> xx (M,6,T), uu (M,2,T), xhat (M,6,T) = x_opt + e^+, err (M,6,T) = dx - e^+ (the last two in `dtype`)."""
    A, B, xp = (a.astype(dtype) for a in jac)
    M, T = x0.shape[0], xo.shape[1]
    K, Lt = np.asarray(KK).astype(dtype), np.asarray(L).astype(dtype)
    xx, uu = np.zeros((M, 6, T)), np.zeros((M, 2, T))
    xhat, err = np.zeros((M, 6, T), dtype), np.zeros((M, 6, T), dtype)
    xx[:, :, 0] = x0
    em = np.zeros((M, 6), dtype) if ehat0 is None else np.broadcast_to(np.asarray(ehat0).astype(dtype), (M, 6)).copy()
    for t in range(T):
        dx = xx[:, :, t] - xo[:, t]
        y = dx if meas is None else dx + meas[:, :, t]
        ep = em + (y.astype(dtype) - em) @ Lt[:, :, t].T
        xhat[:, :, t] = xo[:, t].astype(dtype) + ep
        err[:, :, t] = dx.astype(dtype) - ep
        if t == T - 1:
            break
        e64 = ep.astype(np.float64)
        for r in range(2):
            a = np.zeros(M)
            for c in range(6):
                a = a + KK[r, c, t] * e64[:, c]
            uu[:, r, t] = uo[r, t] + a
        for b in range(M):
            xn = orc.step(mdl, xx[b, :, t], uu[b, :, t])[0]
            xx[b, :, t + 1] = xn if dist is None else xn + dist[b, :, t]
        F = A[t] + B[t] @ K[:, :, t]
        c = xp[t] - xo[:, t + 1].astype(dtype)
        em = ep @ F.T + c
    return xx, uu, xhat, err


def est_stats_of(err):
    """(M,6,T) -> (M,12): max_t |e|, sum_t e^2 in sample order"""
    e = np.asarray(err, dtype=np.float64)
    s = np.zeros((e.shape[0], 6))
    for t in range(e.shape[2]):
        s = s + e[:, :, t] * e[:, :, t]
    return np.concatenate([np.abs(e).max(axis=2), s], axis=1)


def scaled_gap(got, want, xo, uo):
    """The largest gap between two results (xx, uu, xhat, est_stats) scaled per channel by what `want` reaches: states and
    estimates by s_c = max |dx_c|, inputs by max |du_r|, and the statistics of e = dx - e^+ — a difference of two numbers of
    the size of dx — by s_c (the maxima) and s_c^2 (the sums of squares).  A channel whose scale is 0 must agree exactly
    (its gap is then 0, else inf)."""
    gx, gu, gh, gs = (np.asarray(a, dtype=np.longdouble) for a in got)
    wx, wu, wh, ws = (np.asarray(a, dtype=np.longdouble) for a in want)
    T = wx.shape[2]
    sx = np.abs(wx - xo[None]).max(axis=(0, 2)).astype(np.float64)
    su = np.abs(wu - uo[None])[:, :, :T - 1].max(axis=(0, 2)).astype(np.float64)
    ss = np.concatenate([sx, sx ** 2])
    worst = 0.0
    for d, s in ((np.abs(gx - wx).max(axis=(0, 2)), sx), (np.abs(gh - wh).max(axis=(0, 2)), sx),
                 (np.abs(gu - wu).max(axis=(0, 2)), su), (np.abs(gs - ws).max(axis=0), ss)):
        d = d.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(s > 0, d / s, np.where(d == 0, 0.0, np.inf))
        worst = max(worst, float(g.max()))
    return worst


_CACHE = {}


def gains_for(key, mdl, xo, uo, jac):
    """filter_gains about one optimum with the spread of the ensemble tests, from the oracle's Jacobians; computed once"""
    from aircraftoptimalcontrol_amd import batch
    if key not in _CACHE:
        _CACHE[key] = batch.filter_gains(None, xo, uo, np.diag(DELTA_SCALE ** 2), SIGMA, RHO, jac=jac[:2])[0]
    return _CACHE[key]


def selection(B):
    """the members the checker runs: the ends of every tile that exists"""
    return np.array(sorted({b for b in (0, 1, 62, 63, 64, 65, 127, 128, B - 1) if b < B}))


def case_inputs(name, T, B, n_opt):
    """-> sigma, rho, ehat0 (n_opt,6) of a case (None where the case has none)"""
    noise, rho, e0 = CASES[name]
    rng = np.random.default_rng(17)
    rho = np.zeros(6) if rho == "zero" else (RHO if rho else None)
    return (SIGMA if noise else None), rho, (rng.normal(size=(n_opt, 6)) * DELTA_SCALE * 0.5 if e0 else None)


def setup(T, B, nominal=None):
    """optima, gains and members of a size: XO (n,6,T), UO, KK, L (n,6,6,T), jac per optimum, d (B,6), n_opt, mpo, mdl"""
    n_opt, mpo = GEOMETRY[B]
    g, mdl, _ = g4_jacobians()
    if nominal is None:
        XO, UO, KK, jac = windows(n_opt, T)
        L = np.stack([gains_for(("win", k, T), mdl, XO[k], UO[k], jac[k]) for k in range(n_opt)])
    else:
        xo, uo, K1, j1 = nominal
        XO, UO, KK, jac = xo[None], uo[None], K1[None], [j1]
        L = gains_for(("offset", T), mdl, xo, uo, j1)[None]
    return XO, UO, KK, L, jac, deltas(B), n_opt, mpo, mdl


def checker(mdl, XO, UO, KK, L, jac, d, mpo, sel, e0, dist, meas, dtype=np.float64):
    """lqg_loop on the members `sel`, each about its own optimum -> xx, uu, xhat (len(sel),.,T), est_stats (len(sel),12)"""
    out = [[], [], [], []]
    for b in sel:
        k = b // mpo
        xx, uu, xh, err = lqg_loop(mdl, XO[k], UO[k], KK[k], L[k], jac[k], (XO[k][:, 0] + d[b])[None],
                                   None if e0 is None else e0[k], None if dist is None else dist[b][None],
                                   None if meas is None else meas[b][None], dtype)
        for o, v in zip(out, (xx[0], uu[0], xh[0], est_stats_of(err)[0])):
            o.append(v)
    return tuple(np.stack(o) for o in out)


def host_draws(B, T, sigma, rho):
    """what the device draws for members 0 .. B-1 (no GPU at hand): dist, meas (B,6,T) or None"""
    from aircraftoptimalcontrol_amd import mpc
    dist = meas = None
    if sigma is not None:
        dist = np.zeros((B, 6, T))
        for t in range(T - 1):
            dist[:, :, t] = mpc.noise_draws(SEED, t, 0, B, sigma)
    if rho is not None:
        meas = np.stack([mpc.noise_draws(SEED, t, 0, B, rho, 1) for t in range(T)], axis=2)
    return dist, meas


def reference_gap(sizes_T=SIZES_T, sizes_B=tuple(GEOMETRY)):
    """The checker's own rounding: the largest scaled gap between lqg_loop in fp64 and with the estimator in np.longdouble
    over the cases of test_parity_with_the_checker and test_a_nominal_that_is_not_a_rollout, on the host's restatement of
    the device's draws, and over test_parity_at_the_horizon_edges.  Needs no GPU."""
    worst = 0.0
    runs = [(T, B, None) for T in sizes_T for B in sizes_B] + [(33, 65, offset_nominal(33))]
    runs += [(T, EDGE_B, None) for T in EDGE_T]
    for T, B, nominal in runs:
        XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B, nominal)
        sel = selection(B)
        for name in CASES:
            sigma, rho, e0 = case_inputs(name, T, B, n_opt)
            dist, meas = host_draws(B, T, sigma, rho)
            a = checker(mdl, XO, UO, KK, L, jac, d, mpo, sel, e0, dist, meas)
            b = checker(mdl, XO, UO, KK, L, jac, d, mpo, sel, e0, dist, meas, np.longdouble)
            for i, m in enumerate(sel):
                k = m // mpo
                worst = max(worst, scaled_gap([v[i:i + 1] for v in a], [v[i:i + 1] for v in b], XO[k], UO[k]))
    return worst


def _run(XO, UO, KK, L, d, mpo, sigma=None, rho=None, e0=None, trajectories=True, weights=None, **kw):
    from aircraftoptimalcontrol_amd import batch
    g = g4_jacobians()[0]
    bp = _problem(dict(g, xx_opt=XO[0]), weights)
    return batch.track_ensemble(bp, XO, UO, delta=d, KK=KK, members_per_opt=mpo, sigma=sigma, seed=SEED, filter=L, rho=rho,
                                ehat0=e0, trajectories=trajectories, **kw)


def _parity(T, B, nominal=None):
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B, nominal)
    sel = selection(B)
    for name in CASES:
        sigma, rho, e0 = case_inputs(name, T, B, n_opt)
        r = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0)
        assert r["xx_reg"].shape == (B, 6, T) and r["est_stats"].shape == (B, 12) and not r["status"].any()
        draws = rho is not None and bool(np.any(rho))
        assert (sigma is not None) == bool(r["dist"].any()) and draws == bool(r["meas"].any())
        want = checker(mdl, XO, UO, KK, L, jac, d, mpo, sel, e0, r["dist"] if sigma is not None else None,
                       r["meas"] if rho is not None else None)
        worst = 0.0
        for i, m in enumerate(sel):
            k = m // mpo
            got = (r["xx_reg"][m:m + 1], r["uu_reg"][m:m + 1], r["xhat"][m:m + 1], r["est_stats"][m:m + 1])
            worst = max(worst, scaled_gap(got, [v[i:i + 1] for v in want], XO[k], UO[k]))
        print("T = %d, B = %d, %s: scaled gap %.3g (bound %.3g)" % (T, B, name, worst, TOL))
        assert worst <= TOL, (T, B, name, worst)
        if draws:   # the measurement stream is the fourth-word-1 stream of the disturbance's generator
            from aircraftoptimalcontrol_amd import mpc
            for t in (0, T - 1):
                assert np.max(np.abs(r["meas"][:, :, t] - mpc.noise_draws(SEED, t, 0, B, RHO, 1))) <= 1e-13 * RHO.max()
    return r


@pytest.mark.parametrize("B", list(GEOMETRY))
@pytest.mark.parametrize("T", SIZES_T)
def test_parity_with_the_checker(T, B):
    """Windows of g4 with filter_gains' L; T = 3 is the shortest horizon, 17 and 33 end one sample behind a block of 16
    records, 200 spans many; 1, 64, 65 and 130 members are a lone lane, a full tile, a tile and a lane, and three optima.  The
    checker is fed the device's own dist and meas.  Cases: plain; noise; noise + rho; ehat0; rho without disturbance (the
    noise model carries the seed and a sigma of zeros: dist is all zero, meas is not); a rho of six zeros."""
    _parity(T, B)


@pytest.mark.parametrize("T", EDGE_T)
def test_parity_at_the_horizon_edges(T):
    """The parity test at the horizons EDGE_T (see there) with 65 members: both sides of the estimator's block reload.
    Measured on an MI355X: at most 8.2e-15 over the six cases (bound 6.7e-13)."""
    _parity(T, EDGE_B)


KEYS = ("xx_reg", "uu_reg", "xhat", "dist", "meas", "stats", "est_stats", "status")


def shared_stats(r, XO, UO, grp, weights=None):
    """What stats (B,16) must be for the trajectories a call returned: column 8 from batch.traj_cost on a problem whose
    per-trajectory reference is (XO[grp], UO[grp]) with the weights of the call, the others NumPy's subtract / abs / max on
    the fetched xx_reg, uu_reg (tests/test_gpu_ensemble.py numpy_stats)."""
    from aircraftoptimalcontrol_amd import batch
    g = g4_jacobians()[0]
    Q, R, QT = weights if weights is not None else (g["QQt"], g["RRt"], g["QQT"])
    cost = batch.traj_cost(batch.BatchProblem(Q, R, QT, XO[grp], UO[grp], float(g["dt"])), r["xx_reg"], r["uu_reg"])
    return numpy_stats(r["xx_reg"], r["uu_reg"], XO[grp], UO[grp], cost)


def test_shared_statistics_with_a_working_filter():
    """130 members about three optima, T = 33, noise + rho + ehat0, with g4's diagonal weights and with dense ones: the
    sixteen shared statistics are those of the true trajectories about the optimum — the maxima of |dx| and |du|, the final
    dx and first_bad NumPy's on the fetched xx_reg, uu_reg, the cost the bits of aoc_traj_cost with ref = (x_opt, u_opt) —
    although the loop feeds back an estimate that differs from dx.  The weights enter nothing but the cost: every other
    output of the two runs is bit-identical.  The same holds without trajectories (stats, est_stats, status) and without
    any noise (ehat0 alone), with both weights.  Launches the eight fp64-state estimator instances of k_track_ensemble:
    WRITE x NOISE x DIAG."""
    from test_gpu_dense import _tracking_weights
    T, B = 33, 130
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    sigma, rho, e0 = case_inputs("ehat0", T, B, n_opt)
    grp = np.arange(B) // mpo
    dense = _tracking_weights()
    other = [c for c in range(16) if c != 8]
    for sg, rh in ((sigma, rho), (None, None)):                       # NOISE = true, false
        full = {}
        for name, w in (("diag", None), ("dense", dense)):            # DIAG = true, false
            r = full[name] = _run(XO, UO, KK, L, d, mpo, sg, rh, e0, weights=w)           # WRITE = true
            assert not r["status"].any() and np.abs(r["xhat"] - r["xx_reg"]).max() > 1e-4
            assert np.array_equal(r["stats"], shared_stats(r, XO, UO, grp, w)), (name, sg is not None)
            so = _run(XO, UO, KK, L, d, mpo, sg, rh, e0, trajectories=False, weights=w)   # WRITE = false
            assert "xx_reg" not in so and "xhat" not in so
            for k in ("stats", "est_stats", "status"):
                assert np.array_equal(so[k], r[k]), (name, sg is not None, k)
        for k in KEYS:
            if k != "stats":
                assert np.array_equal(full["diag"][k], full["dense"][k]), (sg is not None, k)
        assert np.array_equal(full["diag"]["stats"][:, other], full["dense"]["stats"][:, other])
        assert (full["diag"]["stats"][:, 8] != full["dense"]["stats"][:, 8]).all()


def test_float32_state_storage():
    """f32=True with ehat0 and no noise (the only form the call takes with float32 storage), 130 members, T = 33, diagonal and
    dense weights — the two float32-state estimator instances: every output has the bits of the fp64-storage call, x_reg
    included, since without a disturbance every state from sample 1 on is a float32 value.  With sigma or rho the call is
    refused with its reason."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_dense import _tracking_weights
    T, B = 33, 130
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    _, _, e0 = case_inputs("ehat0", T, B, n_opt)
    for w in (None, _tracking_weights()):
        a = _run(XO, UO, KK, L, d, mpo, None, None, e0, weights=w)
        b = _run(XO, UO, KK, L, d, mpo, None, None, e0, weights=w, f32=True)
        assert np.array_equal(a["xx_reg"][:, :, 1:], a["xx_reg"][:, :, 1:].astype(np.float32)) and not a["status"].any()
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), k
    for sg, rh in ((SIGMA, None), (None, RHO), (SIGMA, RHO)):
        with pytest.raises(batch.AocError, match="float32 state storage .* cannot hold disturbed states"):
            _run(XO, UO, KK, L, d, mpo, sg, rh, e0, f32=True)


OUT_GROUPS = ("xu", "xhat", "dist", "meas")


def abi_call(XO, UO, KK, L, d, mpo, sigma, rho, e0, outputs):
    """One aoc_track_ensemble_lqg call marshalled as batch.track_ensemble marshals it, except that only the output groups
    named in `outputs` (of OUT_GROUPS; "xu" = x_reg and u_reg, which go together) are passed and the others are NULL ->
    dict of the arrays that were passed (xx_reg, uu_reg, xhat, dist, meas: (B,.,T)), stats (B,16), est_stats (B,12),
    status (B,)."""
    import ctypes as C
    import torch
    from aircraftoptimalcontrol_amd import _lib, batch
    bp = _problem(dict(g4_jacobians()[0], xx_opt=XO[0]))
    dev, T, n_opt, B = bp.device, bp.T, XO.shape[0], d.shape[0]
    grp = np.arange(B) // mpo
    nominal = torch.from_numpy(batch.ensemble_nominal(XO, UO, KK)).to(dev)
    filt = batch._filter_to_device(L, n_opt, T, dev)
    x0t = batch.pack_vec(XO[grp, :, 0] + d, dev)
    e0_d = None if e0 is None else batch._dev_f64(np.ascontiguousarray(e0), dev)
    nz = rho_c = None
    if sigma is not None or rho is not None:
        sg = np.zeros(6) if sigma is None else np.asarray(sigma, dtype=np.float64)
        nz = _lib.MpcNoise(SEED, 0, 0, (C.c_double * 6)(*sg.tolist()))
    if rho is not None:
        rho_c = (C.c_double * 6)(*np.asarray(rho, dtype=np.float64).tolist())
    assert set(outputs) <= set(OUT_GROUPS)
    tiled = lambda group, c: batch.alloc_tiled(B, T, c, dev) if group in outputs else None
    buf = dict(xx_reg=tiled("xu", 6), uu_reg=tiled("xu", 2), xhat=tiled("xhat", 6), dist=tiled("dist", 6), meas=tiled("meas", 6))
    nt = batch.ntiles(B)
    stats = torch.empty((nt, _lib.AOC_ENS_NSTAT, batch.TILE), dtype=torch.float64, device=dev)
    est_stats = torch.empty((nt, _lib.AOC_LQG_NSTAT, batch.TILE), dtype=torch.float64, device=dev)
    status = torch.zeros(nt * batch.TILE, dtype=torch.int32, device=dev)
    nbytes = int(_lib.lib().aoc_track_ensemble_lqg_scratch_bytes(n_opt, T))
    scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    p, ptr = bp.c_problem(B), batch._ptr
    _lib.check(_lib.lib().aoc_track_ensemble_lqg(C.byref(p), n_opt, mpo, ptr(nominal), ptr(filt), ptr(x0t), ptr(e0_d),
                                                 C.byref(nz) if nz is not None else None, rho_c, ptr(buf["xx_reg"]),
                                                 ptr(buf["uu_reg"]), ptr(buf["xhat"]), ptr(buf["dist"]), ptr(buf["meas"]),
                                                 ptr(stats), ptr(est_stats), ptr(status), ptr(scratch), nbytes),
               "aoc_track_ensemble_lqg")
    out = {k: batch.unpack(v, B).cpu().numpy() for k, v in buf.items() if v is not None}
    out.update(stats=batch.unpack_vec(stats, B).cpu().numpy(), est_stats=batch.unpack_vec(est_stats, B).cpu().numpy(),
               status=status[:B].cpu().numpy())
    return out


def test_every_output_may_be_null_on_its_own():
    """The C ABI lets (x_reg, u_reg), xhat_reg, dist_out and meas_out be NULL each on its own; the Python call passes all or
    none.  65 members, T = 17, noise + rho + ehat0: with all of them the helper's call has the bits of batch.track_ensemble;
    with xhat alone, meas alone, dist alone, x and u alone, all but x and u, and none, every array that was passed and
    stats, est_stats, status have the bits of the call with all."""
    T, B = 17, 65
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    sigma, rho, e0 = case_inputs("ehat0", T, B, n_opt)
    r = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0)
    full = abi_call(XO, UO, KK, L, d, mpo, sigma, rho, e0, OUT_GROUPS)
    assert sorted(full) == sorted(KEYS)
    for k in KEYS:
        assert np.array_equal(full[k], r[k]), k
    for outputs in (("xhat",), ("meas",), ("dist",), ("xu",), ("xhat", "meas", "dist"), ()):
        got = abi_call(XO, UO, KK, L, d, mpo, sigma, rho, e0, outputs)
        arrays = [k for grp_, ks in (("xu", ("xx_reg", "uu_reg")), ("xhat", ("xhat",)), ("dist", ("dist",)),
                                     ("meas", ("meas",))) if grp_ in outputs for k in ks]
        assert sorted(got) == sorted(arrays + ["stats", "est_stats", "status"]), outputs
        for k in got:
            assert np.array_equal(got[k], full[k]), (outputs, k)


def test_a_rho_of_zeros_is_no_measurement_noise():
    """rho = six zeros beside a disturbance: every output has the bits of the call with rho = NULL, and meas is +0.0
    throughout, no sign bit set."""
    T, B = 33, 130
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    a = _run(XO, UO, KK, L, d, mpo, *case_inputs("noise", T, B, n_opt))
    b = _run(XO, UO, KK, L, d, mpo, *case_inputs("rho_zero", T, B, n_opt))
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert not b["meas"].any() and not np.signbit(b["meas"]).any() and b["dist"].any()


def test_both_streams_follow_step0_and_first():
    """step0 = 7, first = 192, 65 members, T = 17: meas[:, :, t] is the fourth-word-1 stream at step 7 + t of the members
    192 .., dist[:, :, t] the fourth-word-0 stream there (1e-13 of the largest std, the gate of the draws elsewhere in this
    file); the two streams differ in every draw."""
    from aircraftoptimalcontrol_amd import mpc
    T, B = 17, 65
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    r = _run(XO, UO, KK, L, d, mpo, SIGMA, RHO, None, step0=7, first=192)
    assert not r["status"].any()
    for t in range(T):
        assert np.max(np.abs(r["meas"][:, :, t] - mpc.noise_draws(SEED, 7 + t, 192, B, RHO, 1))) <= 1e-13 * RHO.max(), t
    for t in range(T - 1):
        assert np.max(np.abs(r["dist"][:, :, t] - mpc.noise_draws(SEED, 7 + t, 192, B, SIGMA))) <= 1e-13 * SIGMA.max(), t
    assert not r["dist"][:, :, T - 1].any()
    zm, zd = r["meas"][:, :, :T - 1] / RHO[None, :, None], r["dist"][:, :, :T - 1] / SIGMA[None, :, None]
    assert (zm != zd).all()
    # and they are not the draws of step0 = 0, first = 0
    r0 = _run(XO, UO, KK, L, d, mpo, SIGMA, RHO, None)
    assert (r0["meas"] != r["meas"]).all() and (r0["dist"][:, :, :T - 1] != r["dist"][:, :, :T - 1]).all()


def test_a_nominal_that_is_not_a_rollout():
    """c_t != 0: the prior moves although ehat0 = 0 and nothing is measured wrongly"""
    nominal = offset_nominal(33)
    assert np.abs(nominal[3][2] - nominal[0][:, 1:].T).max() > 1e-6
    _parity(33, 65, nominal)


def test_zero_gains_are_the_ensemble_without_feedback():
    """L = 0, rho = None, no ehat0 on g4 (a rollout: c = 0): the estimate stays exactly +0.0, u = u_opt, and every shared
    output equals aoc_track_ensemble on the same nominal with its gains zeroed, bit for bit, with and without disturbance."""
    from aircraftoptimalcontrol_amd import batch
    g, _, T = _g4()
    bp = _problem(g)
    d = deltas(130)
    for sigma in (None, SIGMA):
        r = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, KK=g["KK"], members_per_opt=192, sigma=sigma, seed=SEED,
                                 filter=np.zeros((6, 6, T)), trajectories=True)
        old = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, KK=np.zeros_like(g["KK"]), members_per_opt=192,
                                   sigma=sigma, seed=SEED, trajectories=True)
        for k in ("xx_reg", "uu_reg", "dist", "stats", "status"):
            assert np.array_equal(r[k], old[k]), k
        assert np.array_equal(r["xhat"], np.broadcast_to(g["xx_opt"], r["xhat"].shape)) and not r["meas"].any()
        assert np.array_equal(r["uu_reg"][:, :, :T - 1], np.broadcast_to(g["uu_opt"][:, :T - 1], (130, 2, T - 1)))
        assert np.array_equal(r["max_e"], r["max_dx"])


def test_bits_do_not_depend_on_the_cut_the_tile_the_outputs_or_the_run():
    """130 members about three optima, noise + rho + ehat0, T = 33: the same call again gives the same bits; without
    trajectories the statistics are the same; cut into two calls with first= (members 0-63, 64-129) it gives the bits of one
    call; and the members of the third optimum run alone (n_opt = 1, tile 0) have the bits they had as tile 2 of 3."""
    T, B = 33, 130
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
    sigma, rho, e0 = case_inputs("ehat0", T, B, n_opt)
    keys = ("xx_reg", "uu_reg", "xhat", "dist", "meas", "stats", "est_stats", "status")
    r = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0)
    again = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0)
    for k in keys:
        assert np.array_equal(r[k], again[k]), k
    so = _run(XO, UO, KK, L, d, mpo, sigma, rho, e0, trajectories=False)
    assert "xhat" not in so and "xx_reg" not in so
    for k in ("stats", "est_stats", "status"):
        assert np.array_equal(r[k], so[k]), k
    a = _run(XO[:1], UO[:1], KK[:1], L[:1], d[:64], mpo, sigma, rho, e0[:1], first=0)
    b = _run(XO[1:], UO[1:], KK[1:], L[1:], d[64:], mpo, sigma, rho, e0[1:], first=64)
    for k in keys:
        assert np.array_equal(np.concatenate([a[k], b[k]]), r[k]), k
    c = _run(XO[2:], UO[2:], KK[2:], L[2:], d[128:], mpo, sigma, rho, e0[2:], first=128)
    for k in keys:
        assert np.array_equal(c[k], r[k][128:]), k


def test_leaving_the_domain_is_reported_not_a_fault():
    """The two bad members of tests/test_gpu_ensemble.py (V_0 = -24; a NaN component) among 62 ordinary ones, noise + rho:
    status and first_bad say so, the NaN sticks in the error statistics, and the other lanes keep their bits."""
    T = 33
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, 64)
    clean = _run(XO, UO, KK, L, d, mpo, SIGMA, RHO)
    d2 = d.copy()
    d2[17] = [0, 0, -40, 0, 0, 0]
    d2[40, 4] = np.nan
    assert XO[0, 2, 0] - 40 < 0
    r = _run(XO, UO, KK, L, d2, mpo, SIGMA, RHO)
    assert r["status"][17] & ST_VNONPOS and r["first_bad"][17] == 0
    assert r["status"][40] & ST_NAN and r["first_bad"][40] == 0
    assert np.isnan(r["max_e"][40]).any() and np.isnan(r["sum_e2"][40]).any()
    others = np.setdiff1d(np.arange(64), [17, 40])
    for k in ("xx_reg", "uu_reg", "xhat", "stats", "est_stats", "status"):
        assert np.array_equal(r[k][others], clean[k][others]), k
    assert (clean["first_bad"] == T).all() and not clean["status"].any()


def mc_gains(s):
    """the filter of the Monte Carlo: g4's first MC_T samples, prior spread DELTA_SCALE s, SIGMA, RHO"""
    from aircraftoptimalcontrol_amd import batch
    g, _, (A, B, xp) = g4_jacobians()
    T = MC_T
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    L, _, P_post = batch.filter_gains(None, xo, uo, np.diag((DELTA_SCALE * s) ** 2), SIGMA, RHO, jac=(A[:T - 1], B[:T - 1]))
    return xo, uo, KK, L, P_post


def mc_z(err, P_post):
    """z_cov, z_mean of the sampled estimation error (M,6,T) against the filter's own P_post (6,6,T) and mean 0"""
    M = err.shape[0]
    mean = err.mean(axis=0)
    S = np.einsum("mit,mjt->ijt", err, err) / M - mean[:, None, :] * mean[None, :, :]
    return z_scores(S, mean, P_post, np.zeros_like(mean), M)


@pytest.mark.parametrize("s", [0.1, 1.0])
def test_estimation_error_against_the_filters_own_covariance(s):
    """2048 members, T = 200, SIGMA, rho = 0.1 DELTA_SCALE, spread DELTA_SCALE s: at s = 0.1 the sampled covariance and mean
    of e = dx - e^+ agree with the filter's P^+ and 0 within sampling error (both z <= 5), at s = 1.0 the covariance does
    not (z_cov >= 15): the conditions the CPU checker meets alone (tests/test_lqg_abi.py)."""
    from aircraftoptimalcontrol_amd import batch
    g = _g4()[0]
    xo, uo, KK, L, P_post = mc_gains(s)
    d = mc_members(s)[0]
    r = batch.track_ensemble(_problem(dict(g, xx_opt=xo)), xo, uo, delta=d, KK=KK, sigma=SIGMA, seed=MC_SEED, filter=L, rho=RHO,
                             trajectories=True)
    assert not r["status"].any()
    err = (r["xx_reg"] - xo[None]) - (r["xhat"] - xo[None])
    assert np.allclose(np.abs(err).max(axis=2), r["max_e"], rtol=0, atol=1e-9)
    zc, zm = mc_z(err, P_post)
    rms = np.sqrt(r["sum_e2"].mean(axis=0) / MC_T)
    print("s = %g: z_cov = %.2f, z_mean = %.2f, rms e / rho = %s" % (s, zc, zm, np.round(rms / RHO, 3)))
    if s == 0.1:
        assert zc <= 5 and zm <= 5, (zc, zm)
    else:
        assert zc >= 15, zc


def test_example_prints_the_estimation_error(tmp_path):
    """examples/run_tracking_ensemble.py --rho as a process: one JSON line with the RMS estimation error per channel, that
    of batch.track_ensemble with filter_gains' L for the same seeded members."""
    import json
    from test_gpu_drivers import _run as run_example
    from aircraftoptimalcontrol_amd import batch, problems
    g, _, T = _g4()
    np.save(tmp_path / "xx_star.npy", g["xx_opt"])
    np.save(tmp_path / "uu_star.npy", g["uu_opt"])
    out = run_example("run_tracking_ensemble.py", "--data", tmp_path, "--members", 256, "--seed", 5, "--dt", float(g["dt"]),
                      "--sigma", *SIGMA, "--rho", *RHO)
    lines = out.strip().split("\n")
    line = json.loads(lines[-1])
    assert line["members"] == 256 and line["T"] == T and line["left_the_domain"] == 0
    Q, R, QT = problems.tracking_weights()
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]))
    L = batch.filter_gains(bp, g["xx_opt"], g["uu_opt"], np.diag(DELTA_SCALE ** 2), SIGMA, RHO)[0]
    d = np.random.default_rng(5).normal(size=(256, 6)) * DELTA_SCALE
    r = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, sigma=SIGMA, seed=5, filter=L, rho=RHO)
    assert np.array_equal(np.asarray(line["rho"]), RHO)
    assert np.array_equal(np.asarray(line["rms_estimation_error"]), np.sqrt(r["sum_e2"].mean(axis=0) / T))
