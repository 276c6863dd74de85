"""aoc_filter_gains / batch.filter_gains_device / batch.track_ensemble(filter="device"): the filter Riccati recursion on the
device, for filters that measure all or only some of the six channels.

The checker is joseph_gains below: the Joseph-form recursion with H = the measured rows of the identity, its own Gauss-Jordan
solve, the Jacobians from the oracle (g4_jacobians) — in np.longdouble.  The device computes the same quantities one scalar
measurement at a time (include/aoc.h) with fused multiply-adds and its own sin / cos inside the Jacobians, so the bar is not
bit-identity but a multiple of the reference's OWN rounding: the largest gap between joseph_gains in fp64 and in np.longdouble
over the cases of test_parity_with_the_checker (REF_GAP_*, measured on the CPU by reference_gap below; tests/test_filter_abi.py
pins them), times 16 — the margin of tests/test_gpu_covariance.py and tests/test_gpu_lqg.py.

The metric, with d_i = sqrt(max_t P^-_ii(t)) of the checker: covariances max |D_ij| / (d_i d_j), gains max |DL_ij| d_j / d_i."""
import numpy as np
import pytest

from test_gpu_covariance import MC_SEED, MC_T, g4_jacobians, mc_members, start_moments, windows
from test_gpu_ensemble import DELTA_SCALE, SIGMA, _g4, _problem
from test_gpu_lqg import RHO, mc_z

gpu = pytest.mark.gpu

ST_NAN, ST_VNONPOS, ST_SINGULAR = 1, 2, 4
SIZES_T = (3, 17, 33, 200)
SIZES_N = (1, 3, 65)
# the horizon edges, run at n_opt = 3 alone: T - 1 = 15 and 31 are the last record of a block of the 16-record prefetch (the
# block behind it holds nothing), T = 18 puts one stage into the second block, T = 4 is the first horizon with an inner stage
EDGE_T = (4, 16, 18, 32)
EDGE_N = 3
MASK_T, MASK_N = 17, 3                        # test_every_mask: all 64 sets of measured channels, the full prior, SIGMA
PRIORS = ("small", "unit", "full")            # diag((0.1 DELTA_SCALE)^2), diag(DELTA_SCALE^2), start_moments' full Sigma0
NOISES = (True, False)                        # SIGMA, no disturbance
MEASURED = ((0, 1, 2, 3, 4, 5), (0, 1, 4), (0,))
# The largest gaps (metric above) between joseph_gains in fp64 and in np.longdouble over every case of
# test_parity_with_the_checker, measured by reference_gap(): covariances 1.552e-14 (T = 200, window 32, the full prior, SIGMA,
# {0, 1, 4} measured), gains 5.86e-15 (T = 200, window 63, diag(DELTA_SCALE^2), SIGMA, {0} measured: the unobserved
# directions grow); the device may be 16x that.  (sequential_gains in fp64 stays at 1.11x and 0.98x of them.)
REF_GAP_COV = 1.56e-14
REF_GAP_L = 5.9e-15
TOL_COV, TOL_L = 16 * REF_GAP_COV, 16 * REF_GAP_L


def checked_optima(n_opt):
    """the optima of a call the checker runs: the ends (every one up to three)"""
    return sorted({k for k in (0, 1, 2, n_opt // 2, n_opt - 2, n_opt - 1) if 0 <= k < n_opt})


def prior(name, n_opt):
    """Sigma0 (n_opt,6,6) of a named prior; the full one is cut from start_moments(65), so optimum k has the same prior in
    every call"""
    if name == "full":
        return start_moments(max(SIZES_N))[1][:n_opt]
    return np.broadcast_to(np.diag(((0.1 if name == "small" else 1.0) * DELTA_SCALE) ** 2), (n_opt, 6, 6)).copy()


def gauss_jordan(S, Bm):
    """S^-1 Bm by Gauss-Jordan elimination with partial pivoting, in the dtype of S"""
    n = S.shape[0]
    M = np.concatenate([S, Bm], axis=1).copy()
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for r in range(n):
            if r != k:
                M[r] = M[r] - M[r, k] * M[k]
    return M[:, n:]


def joseph_gains(A, Sigma0, sigma, rho, measured, dtype=np.longdouble):
    """The reference: L = P^- H^T (H P^- H^T + V)^-1, P^+ = (I - L H) P^- (I - L H)^T + L V L^T, P^-' = A P^+ A^T + W in
    `dtype`.  A (T-1,6,6), Sigma0 (6,6), sigma (6,) or None, rho (6,), measured a sequence of channels (may be empty)
    -> L (6,6,T) (unmeasured columns 0), P_prior (6,6,T), P_post (6,6,T)."""
    A = np.asarray(A).astype(dtype)
    T = A.shape[0] + 1
    meas = list(measured)
    I = np.eye(6, dtype=dtype)
    H = I[meas]
    V = np.diag(np.asarray(rho).astype(dtype)[meas] ** 2) if meas else None
    W = np.zeros((6, 6), dtype) if sigma is None else np.diag(np.asarray(sigma).astype(dtype) ** 2)
    P = np.asarray(Sigma0).astype(dtype)
    L, Pm, Pp = (np.zeros((6, 6, T), dtype) for _ in range(3))
    for t in range(T):
        Pm[:, :, t] = P
        post = P
        if meas:
            Ls = gauss_jordan(H @ P @ H.T + V, H @ P).T                # (6,m): P H^T S^-1, S symmetric
            IL = I - Ls @ H
            post = IL @ P @ IL.T + Ls @ V @ Ls.T
            post = (post + post.T) / 2
            L[:, meas, t] = Ls
        Pp[:, :, t] = post
        if t < T - 1:
            P = A[t] @ post @ A[t].T + W
            P = (P + P.T) / 2
    return L, Pm, Pp


def sequential_gains(A, Sigma0, sigma, rho, measured):
    """The recursion of include/aoc.h restated in NumPy fp64: one scalar measurement at a time, multiplicative on the pivot
    row and column.  Same arguments and results as joseph_gains."""
    T = A.shape[0] + 1
    v = np.asarray(rho, dtype=np.float64) ** 2
    W = np.zeros((6, 6)) if sigma is None else np.diag(np.asarray(sigma, dtype=np.float64) ** 2)
    P = np.array(Sigma0, dtype=np.float64)
    L, Pm, Pp = np.zeros((6, 6, T)), np.zeros((6, 6, T)), np.zeros((6, 6, T))
    for t in range(T):
        Pm[:, :, t] = P
        Q = P.copy()
        for c in sorted(measured):
            s = 1.0 / (Q[c, c] + v[c])
            row = Q[c].copy()
            Q = Q - np.outer(row, row) * s
            Q[c, :] = row * (v[c] * s)
            Q[:, c] = row * (v[c] * s)
        Pp[:, :, t] = Q
        for c in measured:
            L[:, c, t] = Q[:, c] / v[c]
        if t < T - 1:
            P = A[t] @ Q @ A[t].T + W
            P = (P + P.T) / 2
    return L, Pm, Pp


def gaps(got, want):
    """(gap of the covariances, gap of the gains) of got = (L, Pm, Pp) against want in the metric of the module docstring.
    An entry whose scale is 0 must agree exactly (its gap is then 0, else inf)."""
    gL, gm, gp = (np.asarray(a, dtype=np.longdouble) for a in got)
    wL, wm, wp = (np.asarray(a, dtype=np.longdouble) for a in want)
    d = np.sqrt(np.abs(np.einsum("iit->it", wm)).max(axis=1)).astype(np.float64)
    dc = np.maximum(np.abs(gm - wm).max(axis=2), np.abs(gp - wp).max(axis=2)).astype(np.float64)
    dl = np.abs(gL - wL).max(axis=2).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.outer(d, d)
        gc = np.where(sc > 0, dc / sc, np.where(dc == 0, 0.0, np.inf))
        sl = d[:, None] / d[None, :]
        gl = np.where(np.isfinite(sl) & (sl > 0), dl / sl, np.where(dl == 0, 0.0, np.inf))
    return float(gc.max()), float(gl.max())


_CACHE = {}


def reference(k, T, pname, noise, measured, dtype=np.longdouble):
    """joseph_gains for window k of g4 (offset 5k) and a case; computed once"""
    key = (k, T, pname, noise, measured, np.dtype(dtype).name)
    if key not in _CACHE:
        A = g4_jacobians()[2][0][5 * k:5 * k + T - 1]
        _CACHE[key] = joseph_gains(A, prior(pname, max(SIZES_N))[k], SIGMA if noise else None, RHO, measured, dtype)
    return _CACHE[key]


def all_cases():
    return [(p, n, m) for p in PRIORS for n in NOISES for m in MEASURED]


def mask_channels(mask):
    """the channels a 6-bit mask of aoc_filter_gains measures, ascending"""
    return tuple(c for c in range(6) if mask >> c & 1)


def reference_gap(sizes_T=SIZES_T, sizes_n=SIZES_N):
    """The reference's own rounding: the largest gaps between joseph_gains in fp64 and in np.longdouble over the cases of
    test_parity_with_the_checker, test_parity_at_the_horizon_edges and test_every_mask -> (cov, L, the case that sets cov,
    the case that sets L).  Needs no GPU."""
    worst = [0.0, 0.0, None, None]
    runs = [(T, k, case) for T in sizes_T for k in sorted({k for n in sizes_n for k in checked_optima(n)}) for case in all_cases()]
    runs += [(T, k, case) for T in EDGE_T for k in checked_optima(EDGE_N) for case in all_cases()]
    runs += [(MASK_T, k, ("full", True, mask_channels(m))) for k in checked_optima(MASK_N) for m in range(64)]
    for T, k, case in runs:
        gc, gl = gaps(reference(k, T, *case, dtype=np.float64), reference(k, T, *case))
        if gc > worst[0]:
            worst[0], worst[2] = gc, (T, k) + case
        if gl > worst[1]:
            worst[1], worst[3] = gl, (T, k) + case
    return tuple(worst)


def _device(XO, UO, S0, noise, measured, **kw):
    from aircraftoptimalcontrol_amd import batch
    g = g4_jacobians()[0]
    bp = _problem(dict(g, xx_opt=XO[0]))
    return batch.filter_gains_device(bp, XO, UO, S0, SIGMA if noise else None, RHO, measured=measured, **kw)


@gpu
@pytest.mark.parametrize("n_opt", SIZES_N)
@pytest.mark.parametrize("T", SIZES_T)
def test_parity_with_the_checker(T, n_opt):
    """Windows of g4 at offsets 5k; T = 3 is the shortest horizon the call takes, 17 and 33 end one sample behind a block of
    the 16-record prefetch, 65 optima are more wavefronts than one; three priors, with and without disturbance, all six
    channels, {0, 1, 4} and {0} measured.  Every unmeasured column of L is exactly +0.0."""
    _parity(T, n_opt, all_cases())


@gpu
@pytest.mark.parametrize("T", EDGE_T)
def test_parity_at_the_horizon_edges(T):
    """The parity test at the horizons EDGE_T (see there) with three optima."""
    _parity(T, EDGE_N, all_cases())


@gpu
def test_every_mask():
    """All 64 sets of measured channels, T = 17, three optima, the full prior, SIGMA: the cross-lane pivots of the measurement
    update run in every order the mask can give them.  The gates of the parity test; every unmeasured column of L is exactly
    +0.0 (all of L with nothing measured) and status is clean.  Measured on an MI355X, this test and the horizon edges
    together: covariances at most 2.7e-15, gains 2.0e-15."""
    _parity(MASK_T, MASK_N, [("full", True, mask_channels(m)) for m in range(64)])


def _parity(T, n_opt, cases):
    XO, UO, _, _ = windows(n_opt, T)
    for pname, noise, measured in cases:
        L, Pm, Pp, status = _device(XO, UO, prior(pname, n_opt), noise, measured)
        assert L.shape == Pm.shape == Pp.shape == (n_opt, 6, 6, T) and not status.any()
        off = [c for c in range(6) if c not in measured]
        assert not L[:, :, off].any() and not np.signbit(L[:, :, off]).any()
        worst = (0.0, 0.0)
        for k in checked_optima(n_opt):
            gc, gl = gaps((L[k], Pm[k], Pp[k]), reference(k, T, pname, noise, measured))
            worst = (max(worst[0], gc), max(worst[1], gl))
        print("T = %d, n_opt = %d, %s, noise %s, measured %s: gap cov %.3g (bound %.3g), L %.3g (bound %.3g)"
              % (T, n_opt, pname, noise, measured, worst[0], TOL_COV, worst[1], TOL_L))
        assert worst[0] <= TOL_COV and worst[1] <= TOL_L, (T, n_opt, pname, noise, measured, worst)


@gpu
def test_bit_exact_identities():
    """P is symmetric; an optimum's records do not depend on n_opt, on its position in the call, on whether cov is NULL, or
    on the run; with nothing measured L = 0, P^+ = P^- and P^- has the bits of aoc_track_covariance on the same nominal
    with its gains set to zero: the time update is one body."""
    import torch
    from aircraftoptimalcontrol_amd import batch
    T, n = 33, 65
    g = g4_jacobians()[0]
    XO, UO, KK, _ = windows(n, T)
    S0 = prior("full", n)
    bp = _problem(dict(g, xx_opt=XO[0]))
    for measured in MEASURED:
        a = _device(XO, UO, S0, True, measured)
        b = _device(XO, UO, S0, True, measured)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        for P in a[1:3]:
            assert np.array_equal(P, P.transpose(0, 2, 1, 3))
        for k in (0, 1, 37, 64):                                        # alone, at position 0 of a call of one
            one = _device(XO[k:k + 1], UO[k:k + 1], S0[k:k + 1], True, measured)
            for x, y in zip(one, a):
                assert np.array_equal(x[0], y[k]), (measured, k)
        rev = _device(XO[::-1], UO[::-1], S0[::-1], True, measured)     # every optimum at another position
        for x, y in zip(rev, a):
            assert np.array_equal(x[::-1], y), measured
        # cov = NULL: the same filter
        nominal = torch.from_numpy(batch.ensemble_nominal(XO, UO, np.zeros_like(KK))).to(bp.device)
        mask = sum(1 << c for c in measured)
        f0, c0, s0 = batch._filter_gains_device(bp, nominal, n, S0, SIGMA, RHO, mask, False)
        f1, c1, s1 = batch._filter_gains_device(bp, nominal, n, S0, SIGMA, RHO, mask, True)
        assert c0 is None and torch.equal(f0, f1) and torch.equal(s0, s1)
        assert np.array_equal(f1.cpu().numpy().reshape(n, T, 6, 6).transpose(0, 2, 3, 1), a[0])
    # nothing measured
    for noise in NOISES:
        L, Pm, Pp, status = _device(XO, UO, S0, noise, ())
        assert not L.any() and not np.signbit(L).any() and np.array_equal(Pm, Pp) and not status.any()
        pred, st = batch.predict_covariance(bp, XO, UO, KK=np.zeros_like(KK), Sigma0=S0, sigma=SIGMA if noise else None)
        assert np.array_equal(np.stack([p["cov_dx"] for p in pred]), Pm) and not st.any()
        assert np.abs(Pm[:, :, :, -1]).max() > 0


@gpu
def test_the_filter_filters():
    """diag P^+ <= diag P^-; diag P^+ < rho^2 on measured channels; L_t (P^-_t + V) = P^-_t to 1e-10 where all six are
    measured (the test of batch.filter_gains)."""
    T = 200
    XO, UO, _, _ = windows(3, T)
    V = np.diag(RHO ** 2)
    for pname in PRIORS:
        for measured in MEASURED:
            L, Pm, Pp, status = _device(XO, UO, prior(pname, 3), True, measured)
            dm, dp = np.einsum("kiit->kit", Pm), np.einsum("kiit->kit", Pp)
            assert not status.any() and (dp <= dm).all() and (dp > 0).all()
            assert (dp[:, list(measured)] < (RHO ** 2)[None, list(measured), None]).all()
            if len(measured) == 6:
                for k in range(3):
                    for t in range(T):
                        assert np.allclose(L[k, :, :, t] @ (Pm[k, :, :, t] + V), Pm[k, :, :, t], rtol=1e-10, atol=1e-18)


@gpu
def test_an_indefinite_prior_is_a_status_not_a_fault():
    """A Sigma0 with a negative eigenvalue (a pivot Q_00 + v_0 < 0) in optimum 1 of three sets AOC_ST_SINGULAR there and
    leaves the other two bit-identical to a call without it."""
    T = 33
    XO, UO, _, _ = windows(3, T)
    S0 = prior("unit", 3)
    clean = _device(XO, UO, S0, True, MEASURED[0])
    assert not clean[3].any()
    bad = S0.copy()
    bad[1, 0, 0] = -4.0 * RHO[0] ** 2
    assert np.linalg.eigvalsh(bad[1]).min() < 0 and bad[1, 0, 0] + RHO[0] ** 2 < 0
    got = _device(XO, UO, bad, True, MEASURED[0])
    assert got[3][1] & ST_SINGULAR and got[3][0] == 0 and got[3][2] == 0
    for x, y in zip(got[:3], clean[:3]):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2])
    assert not np.array_equal(got[0][1], clean[0][1])


@gpu
def test_the_device_route_is_the_host_route_with_the_same_gains():
    """track_ensemble(filter="device") equals, bit for bit, track_ensemble(filter=L) with the same L read back: 130 members
    about three optima, noise, rho, with all six channels and with {0, 1, 4} measured."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_ensemble import deltas
    T, B, mpo = 33, 130, 64
    g = g4_jacobians()[0]
    XO, UO, KK, _ = windows(3, T)
    S0 = prior("full", 3)
    bp = _problem(dict(g, xx_opt=XO[0]))
    kw = dict(delta=deltas(B), KK=KK, members_per_opt=mpo, sigma=SIGMA, seed=11, rho=RHO, trajectories=True)
    for measured in (None, (0, 1, 4)):
        L = batch.filter_gains_device(bp, XO, UO, S0, SIGMA, RHO, measured=measured)[0]
        dev = batch.track_ensemble(bp, XO, UO, filter="device", Sigma0=S0, measured=measured, **kw)
        host = batch.track_ensemble(bp, XO, UO, filter=L, **kw)
        assert not dev["filter_status"].any() and not dev["status"].any()
        for k in ("xx_reg", "uu_reg", "xhat", "dist", "meas", "stats", "est_stats", "status"):
            assert np.array_equal(dev[k], host[k]), (measured, k)
        assert np.abs(dev["xhat"] - dev["xx_reg"]).max() > 0


@gpu
def test_estimation_error_against_the_devices_own_covariance():
    """The Monte Carlo of tests/test_gpu_lqg.py with the device's gains: 2048 members, T = 200, SIGMA, rho = 0.1 DELTA_SCALE,
    spread 0.1 DELTA_SCALE, all channels measured: the sampled covariance and mean of e = dx - e^+ agree with the device's
    own P^+ and 0 within sampling error (z_cov, z_mean <= 5; the host's gains give 3.5)."""
    from aircraftoptimalcontrol_amd import batch
    g = _g4()[0]
    T, s = MC_T, 0.1
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    S0 = np.diag((DELTA_SCALE * s) ** 2)
    bp = _problem(dict(g, xx_opt=xo))
    P_post = batch.filter_gains_device(bp, xo, uo, S0, SIGMA, RHO)[2][0]
    r = batch.track_ensemble(bp, xo, uo, delta=mc_members(s)[0], KK=KK, sigma=SIGMA, seed=MC_SEED, filter="device", Sigma0=S0,
                             rho=RHO, trajectories=True)
    assert not r["status"].any() and not r["filter_status"].any()
    err = (r["xx_reg"] - xo[None]) - (r["xhat"] - xo[None])
    zc, zm = mc_z(err, P_post)
    print("z_cov = %.2f, z_mean = %.2f" % (zc, zm))
    assert zc <= 5 and zm <= 5, (zc, zm)


@gpu
def test_example_with_device_gains(tmp_path):
    """examples/run_tracking_ensemble.py --rho ... --device-gains [--measured c ...] as a process: the line that
    track_ensemble(filter="device") gives for the same seeded members."""
    import json
    from test_gpu_drivers import _run as run_example
    from aircraftoptimalcontrol_amd import batch, problems
    g, _, T = _g4()
    np.save(tmp_path / "xx_star.npy", g["xx_opt"])
    np.save(tmp_path / "uu_star.npy", g["uu_opt"])
    Q, R, QT = problems.tracking_weights()
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]))
    d = np.random.default_rng(5).normal(size=(256, 6)) * DELTA_SCALE
    for extra, measured in (((), None), (("--measured", 0, 1, 4), (0, 1, 4))):
        out = run_example("run_tracking_ensemble.py", "--data", tmp_path, "--members", 256, "--seed", 5, "--dt", float(g["dt"]),
                          "--sigma", *SIGMA, "--delta", *DELTA_SCALE, "--rho", *RHO, "--device-gains", *extra)
        line = json.loads(out.strip().split("\n")[-1])
        r = batch.track_ensemble(bp, g["xx_opt"], g["uu_opt"], delta=d, sigma=SIGMA, seed=5, filter="device",
                                 Sigma0=np.diag(DELTA_SCALE ** 2), rho=RHO, measured=measured)
        assert line["members"] == 256 and line["T"] == T and line["device_gains"] is True
        assert line["measured"] == list(measured if measured is not None else range(6))
        assert np.array_equal(np.asarray(line["rms_estimation_error"]), np.sqrt(r["sum_e2"].mean(axis=0) / T))
