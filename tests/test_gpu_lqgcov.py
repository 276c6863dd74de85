"""aoc_track_covariance_lqg / batch.predict_covariance_lqg / batch.track_ensemble(filter=, predict_joint=True): what linear
theory predicts for the LQG loop — the joint moments of dx and of the posterior estimation error e.

The checker is numpy_joint below: the recursion of include/aoc.h in NumPy with A, B and the stepped state from the oracle's
Dynamics.step, in np.longdouble.  The device differs from it in the order of the sums, in fused multiply-adds, in N = F - A
instead of B K and in its own sin / cos inside the Jacobians, so the bar is not bit-identity but a multiple of the checker's
OWN rounding: the largest gap between numpy_joint in fp64 and in np.longdouble over the cases of the parity tests (REF_GAP,
measured on the CPU by reference_gap below; tests/test_lqgcov_abi.py pins it), times 16 — the margin of the sibling files.

The metric (gaps below), with dX_i = sqrt(max_t X_ii) and dE_i = sqrt(max_t E_ii) of the checker: X over dX_i dX_j, E over
dE_i dE_j, C_ij over dX_i dE_j, m over dX, mu over dE, the mean of du over s_r = sqrt(max_t cov(du)_rr) and its covariance
over s_r s_s.  One exception, written down here because no fp64 code can meet the rule without it: with L = 0 the estimate
never moves, cov(e^+) = X - C - C^T + E is 0 in exact arithmetic and what any implementation returns for the moments of du is
the rounding of that cancellation, of the size eps (dX + dE)^2 — its own maximum is no scale.  There (case "zero") the scale
of du is the bound s_r = sum_j max_t |K_rj| (dX_j + dE_j), the largest du_r the loop could produce from states of that size."""
import numpy as np
import pytest

from test_gpu_covariance import (EDGE_N, EDGE_T, G13_BOUND, MC_M, MC_SEED, MC_T, TRI, g4_jacobians, g13_gains, g13_gap,
                                 g13_optima, g13_problem, g13_report, mc_members, offset_nominal, start_moments, windows,
                                 z_scores)
from test_gpu_ensemble import DELTA_SCALE, SIGMA, _g4, _problem
from test_gpu_filter import checked_optima, sequential_gains
from test_gpu_lqg import RHO, mc_gains

gpu = pytest.mark.gpu

ST_NAN, ST_VNONPOS = 1, 2
SIZES_T = (3, 17, 33, 200)
SIZES_N = (1, 3, 65)
NREC = 96
# case -> (gains: channels measured by the filter that made them, or None for L = 0; the factor on rho the gains were made
# with; W; V; moments: "kalman" = diag prior, ehat0 = mean0, "full" = start_moments' Sigma0 and ehat0 != mean0 != 0)
CASES = {
    "kalman":   ((0, 1, 2, 3, 4, 5), 1.0, True, True, "kalman"),
    "meas014":  ((0, 1, 4), 1.0, True, True, "kalman"),
    "meas0":    ((0,), 1.0, True, True, "kalman"),
    "detuned":  ((0, 1, 2, 3, 4, 5), 4.0, True, True, "full"),
    "zero":     (None, 1.0, True, True, "kalman"),
    "no_W":     ((0, 1, 2, 3, 4, 5), 1.0, False, True, "full"),
    "no_rho":   ((0, 1, 2, 3, 4, 5), 1.0, True, False, "full"),
}
# The largest gap (metric above) between numpy_joint in fp64 and in np.longdouble over every case of
# test_parity_with_the_checker and test_a_nominal_that_is_not_a_rollout, measured by reference_gap(): 1.822e-12, set by X of
# the case "zero" at T = 200, window 2 (L = 0: nothing is fed back but the prior, and X' = A X A^T + W is what is left of four
# terms that cancel); the device may be 16x that.
REF_GAP = 1.83e-12
REF_GAP_CASE = (200, 2, "zero", "X")
TOL = 16 * REF_GAP
# orthogonality of estimate and error with the Kalman gains of a consistent prior (spread s DELTA_SCALE, SIGMA, RHO, ehat0 =
# mean0, the first MC_T samples of g4): the gaps E_t - P^+_t and C_t - E_t of numpy_joint in fp64 on sequential_gains' L and
# P^+, in the dE metric; the device, on its own gains and P^+, may be 16x that.  Measured by orthogonality_gap().
# Measured: E 2.60e-16 and C 3.79e-15 at s = 0.1, E 2.74e-16 and C 6.16e-14 at s = 1.0.
ORTH_E = {0.1: 2.7e-16, 1.0: 2.8e-16}
ORTH_C = {0.1: 3.8e-15, 1.0: 6.2e-14}


def numpy_joint(jac, xo, KK, L, mean0=None, ehat0=None, Sigma0=None, sigma=None, rho=None, dtype=np.float64):
    """The recursion of include/aoc.h for ONE optimum: jac = jacobians(...) (A, B, stepped state), xo (6,T), KK (2,6,T),
    L (6,6,T), mean0, ehat0 (6,), Sigma0 (6,6), sigma, rho (6,) (None = 0 each) -> records (T,96) in `dtype`."""
    A, B, xp = (np.asarray(a).astype(dtype) for a in jac)
    T = xo.shape[1]
    K, Lt = np.asarray(KK).astype(dtype), np.asarray(L).astype(dtype)
    z6 = np.zeros(6, dtype)
    m = z6 if mean0 is None else np.asarray(mean0).astype(dtype)
    mu = m - (z6 if ehat0 is None else np.asarray(ehat0).astype(dtype))
    S0 = np.zeros((6, 6), dtype) if Sigma0 is None else np.asarray(Sigma0).astype(dtype)
    W = np.zeros((6, 6), dtype) if sigma is None else np.diag(np.asarray(sigma).astype(dtype) ** 2)
    V = np.zeros((6, 6), dtype) if rho is None else np.diag(np.asarray(rho).astype(dtype) ** 2)
    X, Cm, Em = S0, S0, S0
    I = np.eye(6, dtype=dtype)
    rec = np.zeros((T, NREC), dtype)
    for t in range(T):
        J = I - Lt[:, :, t]
        mu = J @ mu
        E = J @ Em @ J.T + Lt[:, :, t] @ V @ Lt[:, :, t].T
        E = (E + E.T) / 2
        Cx = Cm @ J.T
        rec[t, 0:6], rec[t, 6:12] = m, mu
        rec[t, 12:33] = [X[i, j] for i, j in TRI]
        rec[t, 33:54] = [E[i, j] for i, j in TRI]
        rec[t, 54:90] = Cx.reshape(36)
        if t == T - 1:
            break
        Kt = K[:, :, t]
        rec[t, 90:92] = Kt @ (m - mu)
        KHK = Kt @ (X - Cx - Cx.T + E) @ Kt.T
        rec[t, 92:95] = KHK[0, 0], KHK[0, 1], KHK[1, 1]
        N = B[t] @ Kt
        F = A[t] + N
        c = xp[t] - xo[:, t + 1].astype(dtype)
        m = F @ m - N @ mu + c
        mu = A[t] @ mu
        Xn = F @ X @ F.T - F @ Cx @ N.T - N @ Cx.T @ F.T + N @ E @ N.T + W
        Cm = (F @ Cx - N @ E) @ A[t].T + W
        Em = A[t] @ E @ A[t].T + W
        X, Em = (Xn + Xn.T) / 2, (Em + Em.T) / 2
    return rec


def unpack(rec):
    """records (T,96) -> m (T,6), mu (T,6), X, E, C (T,6,6), mean du (T,2), cov du (T,3) in the records' dtype"""
    rec = np.asarray(rec)
    T = rec.shape[0]
    X, E = np.zeros((T, 6, 6), rec.dtype), np.zeros((T, 6, 6), rec.dtype)
    for n, (i, j) in enumerate(TRI):
        X[:, i, j] = X[:, j, i] = rec[:, 12 + n]
        E[:, i, j] = E[:, j, i] = rec[:, 33 + n]
    return rec[:, 0:6], rec[:, 6:12], X, E, rec[:, 54:90].reshape(T, 6, 6), rec[:, 90:92], rec[:, 92:95]


def du_bound(want, KK):
    """the scale of du where its own maximum is none (module docstring): s_r = sum_j max_t |K_rj| (dX_j + dE_j)"""
    _, _, X, E, _, _, _ = unpack(np.asarray(want, dtype=np.float64))
    d = np.sqrt(np.abs(np.einsum("tii->ti", X)).max(axis=0)) + np.sqrt(np.abs(np.einsum("tii->ti", E)).max(axis=0))
    return np.abs(np.asarray(KK, dtype=np.float64)).max(axis=2) @ d


def gaps(got, want, du_scale=None):
    """The gaps between two records (T,96) in the metric of the module docstring -> dict(m, mu, X, E, C, du_mean, du_cov).
    An entry whose scale is 0 must agree exactly (its gap is then 0, else inf)."""
    g, w = (unpack(np.asarray(a, dtype=np.longdouble)) for a in (got, want))
    w64 = unpack(np.asarray(want, dtype=np.float64))
    dX = np.sqrt(np.abs(np.einsum("tii->ti", w64[2])).max(axis=0))
    dE = np.sqrt(np.abs(np.einsum("tii->ti", w64[3])).max(axis=0))
    su = np.sqrt(np.abs(w64[6][:, [0, 2]]).max(axis=0)) if du_scale is None else np.asarray(du_scale, dtype=np.float64)
    scales = dict(m=dX, mu=dE, X=np.outer(dX, dX), E=np.outer(dE, dE), C=np.outer(dX, dE), du_mean=su,
                  du_cov=np.array([su[0] ** 2, su[0] * su[1], su[1] ** 2]))
    out = {}
    for n, (name, sc) in enumerate(scales.items()):
        d = np.abs(g[n] - w[n]).max(axis=0).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = float(np.where(sc > 0, d / sc, np.where(d == 0, 0.0, np.inf)).max())
    return out


def case_moments(name, k):
    """-> mean0, ehat0, Sigma0 of optimum k in a case; cut from arrays of max(SIZES_N) optima, so optimum k has the same in
    every call"""
    m0, S0 = start_moments(max(SIZES_N))
    if CASES[name][4] == "kalman":
        return m0[k], m0[k], np.diag(DELTA_SCALE ** 2)
    e0 = np.random.default_rng(17).normal(size=(max(SIZES_N), 6)) * DELTA_SCALE * 0.5
    return m0[k], e0[k], S0[k]


def case_noise(name):
    """-> sigma, rho of the prediction (None where the case has none)"""
    _, _, w, v, _ = CASES[name]
    return (SIGMA if w else None), (RHO if v else None)


def host_gains(name, A, Sigma0):
    """the gains of a case without a GPU: the sequential form of aoc_filter_gains restated in NumPy (test_gpu_filter.py)"""
    measured, factor, w, _, _ = CASES[name]
    T = A.shape[0] + 1
    if measured is None:
        return np.zeros((6, 6, T))
    return sequential_gains(A, Sigma0, SIGMA if w else None, factor * RHO, measured)[0]


def reference(jac, xo, KK, L, m0, e0, S0, sigma, rho, dtype=np.longdouble):
    return numpy_joint(jac, xo, KK, L, m0, e0, S0, sigma, rho, dtype)


def all_gaps(got, want, name, KK):
    return gaps(got, want, du_bound(want, KK) if name == "zero" else None)


def reference_gap(sizes_T=SIZES_T, sizes_n=SIZES_N):
    """The checker's own rounding: the largest gap between numpy_joint in fp64 and in np.longdouble over the cases of
    test_parity_with_the_checker, test_parity_at_the_horizon_edges (EDGE_T of tests/test_gpu_covariance.py, three optima)
    and test_a_nominal_that_is_not_a_rollout, on host_gains' L -> (gap, the case that sets it).  Needs no GPU."""
    worst, which = 0.0, None

    def one(tag, name, jac, xo, KK, k):
        nonlocal worst, which
        m0, e0, S0 = case_moments(name, k)
        sigma, rho = case_noise(name)
        L = host_gains(name, jac[0], S0)
        g = all_gaps(numpy_joint(jac, xo, KK, L, m0, e0, S0, sigma, rho), reference(jac, xo, KK, L, m0, e0, S0, sigma, rho),
                     name, KK)
        for part, v in g.items():
            if v > worst:
                worst, which = v, tag + (name, part)
    for T in tuple(sizes_T) + EDGE_T:
        ks = checked_optima(EDGE_N) if T in EDGE_T else sorted({k for n in sizes_n for k in checked_optima(n)})
        XO, _, KK, jac = windows(max(ks) + 1, T)
        for k in ks:
            for name in CASES:
                one((T, k), name, jac[k], XO[k], KK[k], k)
    xo, _, K1, j1 = offset_nominal(33)
    for name in ("kalman", "detuned"):
        one(("offset", 0), name, j1, xo, K1, 0)
    return worst, which


def orthogonality_gap(s, L=None, P_post=None, got=None):
    """(gap of E_t against P^+_t, gap of C_t against E_t) in the dE metric, on the first MC_T samples of g4 with the prior
    spread s DELTA_SCALE, SIGMA, RHO, ehat0 = mean0: of numpy_joint in fp64 on sequential_gains' L and P^+ (no GPU), or of
    the records `got` with the P_post (6,6,T) they belong to."""
    g, _, (A, B, xp) = g4_jacobians()
    T = MC_T
    S0 = np.diag((DELTA_SCALE * s) ** 2)
    if got is None:
        L, _, P_post = sequential_gains(A[:T - 1], S0, SIGMA, RHO, tuple(range(6)))
        got = numpy_joint((A[:T - 1], B[:T - 1], xp[:T - 1]), g["xx_opt"][:, :T], g["KK"][:, :, :T], L, None, None, S0, SIGMA, RHO)
    _, _, _, E, Cx, _, _ = unpack(np.asarray(got, dtype=np.float64))
    Pp = np.asarray(P_post, dtype=np.float64).transpose(2, 0, 1)
    dE = np.sqrt(np.abs(np.einsum("tii->ti", Pp)).max(axis=0))
    sc = np.outer(dE, dE)
    return float((np.abs(E - Pp).max(axis=0) / sc).max()), float((np.abs(Cx - E).max(axis=0) / sc).max())


def joint_z(dx, err, du, p):
    """z-scores of sampled dx, e (M,6,T) and du (M,2,T-1) against a prediction p (lqg_covariance_moments' dict) ->
    dict(dx=(z_cov, z_mean), e=..., du=..., cross=z): z_scores of test_gpu_covariance.py, and for the cross term
    |S_ij - C_ij| / sqrt((X_ii E_jj + C_ij C_ji) / M)"""
    M = dx.shape[0]

    def moments(a):
        mean = a.mean(axis=0)
        return np.einsum("mit,mjt->ijt", a, a) / M - mean[:, None, :] * mean[None, :, :], mean
    out = {}
    Sx, mx = moments(dx)
    out["dx"] = z_scores(Sx, mx, p["cov_dx"], p["mean_dx"], M)
    Se, me = moments(err)
    out["e"] = z_scores(Se, me, p["cov_e"], p["mean_e"], M)
    Su, mu = moments(du)
    T1 = du.shape[2]
    d = np.einsum("iit->it", p["cov_du"][:, :, :T1])
    with np.errstate(divide="ignore", invalid="ignore"):
        zc = np.abs(Su - p["cov_du"][:, :, :T1]) / np.sqrt((d[:, None] * d[None, :] + p["cov_du"][:, :, :T1] ** 2) / M)
        zm = np.abs(mu - p["mean_du"][:, :T1]) / np.sqrt(d / M)
    out["du"] = (float(np.nanmax(zc)), float(np.nanmax(zm)))
    Sc = np.einsum("mit,mjt->ijt", dx, err) / M - mx[:, None, :] * me[None, :, :]
    Cx = p["cov_dx_e"]
    dX, dE = np.einsum("iit->it", p["cov_dx"]), np.einsum("iit->it", p["cov_e"])
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.abs(Sc - Cx) / np.sqrt((dX[:, None, :] * dE[None, :, :] + Cx * Cx.transpose(1, 0, 2)) / M)
    out["cross"] = float(np.nanmax(z))
    return out


# ---------------------------------------------------------------------------------------------------------------------
def _bp(XO):
    return _problem(dict(g4_jacobians()[0], xx_opt=XO[0]))


def _device_gains(name, bp, XO, UO, S0):
    """the gains of a case from aoc_filter_gains -> L (n,6,6,T) on the host"""
    from aircraftoptimalcontrol_amd import batch
    measured, factor, w, _, _ = CASES[name]
    n, T = XO.shape[0], XO.shape[2]
    if measured is None:
        return np.zeros((n, 6, 6, T))
    L, _, _, st = batch.filter_gains_device(bp, XO, UO, S0, SIGMA if w else None, factor * RHO, measured=measured)
    assert not st.any()
    return L


def _predict(bp, XO, UO, KK, L, m0, e0, S0, sigma, rho):
    from aircraftoptimalcontrol_amd import batch
    pred, status = batch.predict_covariance_lqg(bp, XO, UO, L, KK=KK, mean0=m0, ehat0=e0, Sigma0=S0, sigma=sigma, rho=rho)
    return np.stack([p["raw"] for p in pred]), status, pred


def _case_call(name, XO, UO, KK):
    n = XO.shape[0]
    bp = _bp(XO)
    mom = [case_moments(name, k) for k in range(n)]
    m0, e0, S0 = (np.stack([m[i] for m in mom]) for i in range(3))
    sigma, rho = case_noise(name)
    L = _device_gains(name, bp, XO, UO, S0)
    got, status, pred = _predict(bp, XO, UO, KK, L, m0, e0, S0, sigma, rho)
    return got, status, pred, L, (m0, e0, S0, sigma, rho)


@gpu
@pytest.mark.parametrize("n_opt", SIZES_N)
@pytest.mark.parametrize("T", SIZES_T)
def test_parity_with_the_checker(T, n_opt):
    """Windows of g4 at offsets 5k; T = 3 is the shortest horizon the call takes, 17 and 33 end one sample behind a block of
    the 16-sample prefetch, 65 optima are more wavefronts than one.  The cases of CASES: the Kalman gains of aoc_filter_gains
    with all channels, {0, 1, 4} and {0} measured, a detuned filter (the gains of 4 rho applied with rho, ehat0 != mean0 != 0,
    a full Sigma0), L = 0, without W, without rho.  The checker runs on the very L the device was handed."""
    _parity(T, n_opt)


@gpu
@pytest.mark.parametrize("T", EDGE_T)
def test_parity_at_the_horizon_edges(T):
    """The parity test at the horizons EDGE_T of tests/test_gpu_covariance.py (both sides of the 16-sample prefetch's block
    edge, a block of one stage, the first inner stage) with three optima."""
    _parity(T, EDGE_N)


def _parity(T, n_opt):
    XO, UO, KK, jac = windows(n_opt, T)
    for name in CASES:
        got, status, pred, L, (m0, e0, S0, sigma, rho) = _case_call(name, XO, UO, KK)
        assert got.shape == (n_opt, T, NREC) and not status.any()
        worst = {}
        for k in checked_optima(n_opt):
            want = reference(jac[k], XO[k], KK[k], L[k], m0[k], e0[k], S0[k], sigma, rho)
            for part, v in all_gaps(got[k], want, name, KK[k]).items():
                worst[part] = max(worst.get(part, 0.0), v)
        print("T = %d, n_opt = %d, %s: %s (bound %.3g)" % (T, n_opt, name, {p: "%.3g" % v for p, v in worst.items()}, TOL))
        assert max(worst.values()) <= TOL, (T, n_opt, name, worst)
        tail = got[:, T - 1, 90:]
        assert not tail.any() and not np.signbit(tail).any() and not np.signbit(got[:, :, 95]).any() and not got[:, :, 95].any()
    # the unpacked form is the record
    from aircraftoptimalcontrol_amd import batch
    p = batch.lqg_covariance_moments(got[0])
    m, mu, X, E, Cx, um, uc = unpack(got[0])
    assert np.array_equal(p["mean_dx"], m.T) and np.array_equal(p["mean_e"], mu.T) and np.array_equal(p["mean_du"], um.T)
    assert np.array_equal(p["cov_dx"], X.transpose(1, 2, 0)) and np.array_equal(p["cov_e"], E.transpose(1, 2, 0))
    assert np.array_equal(p["cov_dx_e"], Cx.transpose(1, 2, 0)) and np.array_equal(p["cov_du"][0, 1], uc[:, 1])
    assert np.array_equal(p["cov_xhat"], (X - Cx - Cx.transpose(0, 2, 1) + E).transpose(1, 2, 0))
    assert np.array_equal(pred[0]["cov_dx_e"], p["cov_dx_e"])


@gpu
def test_a_nominal_that_is_not_a_rollout():
    """c_t != 0: the mean of dx moves although mean0 = ehat0, the mean of e does not feel it (separation)"""
    T = 33
    xo, uo, KK, jac = offset_nominal(T)
    for name in ("kalman", "detuned"):
        got, status, _, L, (m0, e0, S0, sigma, rho) = _case_call(name, xo[None], uo[None], KK[None])
        want = reference(jac, xo, KK, L[0], m0[0], e0[0], S0[0], sigma, rho)
        g = all_gaps(got[0], want, name, KK)
        print("offset nominal, %s: %s (bound %.3g)" % (name, {p: "%.3g" % v for p, v in g.items()}, TOL))
        assert max(g.values()) <= TOL and not status.any()
        assert np.abs(got[0, 1:, 0:6]).max() > 1e-6
        if name == "kalman":   # ehat0 = mean0: the error starts with mean 0 and neither c nor dx enters it
            assert not got[0, :, 6:12].any()


@gpu
def test_stage_records_at_wide_angles():
    """Both k_cov_stage instances off the g4 fixture, read through aoc_track_covariance_lqg alone: three-sample optima on all
    216 points of G13 (g13_optima of tests/test_gpu_covariance.py), filter = 0, mean0 = e_j, no Sigma0, no noise, no rho.
    Setting (a), ehat0 = 0: the error starts at mu_0 = e_j and entries 6-11 of sample 1 are mu_1 = A[:, j], the record of
    k_cov_stage<false>: against the golden fx per entry over |A_ij|, bound 1e-12 (the gate of aoc_step_batch on these
    Jacobians), zero outside A's sparsity — and with the bits they have when the nominal carries the seeded K instead of
    K = 0: a filter knows its input.  Setting (b), ehat0 = mean0 = e_j with the seeded K: mu = 0 and entries 0-5 of sample 1
    are m_1 = F[:, j] of k_cov_stage<true>, against A + B K over |A_ij| + sum_r |B_ir K_rj|, the same bound.  status as in
    tests/test_gpu_covariance.py.
    Measured on an MI355X: (a) 3.92e-13; (b) 3.49e-13, both at entry (2, 2) of point 133."""
    from test_gpu_parity import _record
    K = g13_gains()
    g, XO, UO, KK, A, B = g13_optima(K)
    n = XO.shape[0]
    bp = g13_problem(g)
    L = np.zeros((n, 6, 6, 3))
    want_status = np.where(XO[:, 2, 1] <= 0, ST_VNONPOS, 0)
    Amu, Amu0, F = np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for j in range(6):
        e = np.eye(6)[j]
        a, st, _ = _predict(bp, XO, UO, KK, L, e, None, None, None, None)                      # (a), the seeded K
        a0, st0, _ = _predict(bp, XO, UO, np.zeros_like(KK), L, e, None, None, None, None)     # (a), K = 0
        b, stb, _ = _predict(bp, XO, UO, KK, L, e, e, None, None, None)                        # (b)
        Amu[:, :, j], Amu0[:, :, j], F[:, :, j] = a[:, 1, 6:12], a0[:, 1, 6:12], b[:, 1, 0:6]
        assert np.array_equal(a[:, 0, 6:12], np.broadcast_to(e, (n, 6))) and not b[:, :2, 6:12].any()
        for s in (st, st0, stb):
            assert np.array_equal(s, want_status), j
    assert np.array_equal(Amu, Amu0)
    gap_a, point_a, entry_a = g13_gap(Amu, A, B)
    gap_b, point_b, entry_b = g13_gap(F, A, B, K)
    rec = dict(points=n, A=g13_report("mu_1 = A through aoc_track_covariance_lqg", gap_a, point_a, entry_a, g),
               F=g13_report("m_1 = A + B K through aoc_track_covariance_lqg", gap_b, point_b, entry_b, g))
    _record("g13_lqgcov_stage.json", rec)
    assert gap_a <= G13_BOUND and gap_b <= G13_BOUND, (gap_a, point_a, entry_a, gap_b, point_b, entry_b)


@gpu
def test_bit_exact_identities():
    """X and E come from their upper triangles; the same record for an optimum alone, at another position and in a second
    run; with no Sigma0, no noise and no rho every covariance entry is exactly +0.0; filter="device" is filter=L with the
    same L read back."""
    from aircraftoptimalcontrol_amd import batch
    T, n = 33, 65
    XO, UO, KK, _ = windows(n, T)
    bp = _bp(XO)
    for name in ("meas014", "detuned"):
        a, st, _, L, (m0, e0, S0, sigma, rho) = _case_call(name, XO, UO, KK)
        b, _, _ = _predict(bp, XO, UO, KK, L, m0, e0, S0, sigma, rho)
        assert np.array_equal(a, b) and not st.any()
        for k in (0, 1, 37, 64):
            one, _, _ = _predict(_bp(XO[k:k + 1]), XO[k:k + 1], UO[k:k + 1], KK[k:k + 1], L[k:k + 1], m0[k:k + 1], e0[k:k + 1],
                                 S0[k:k + 1], sigma, rho)
            assert np.array_equal(one[0], a[k]), (name, k)
        rev, _, _ = _predict(bp, XO[::-1], UO[::-1], KK[::-1], L[::-1], m0[::-1], e0[::-1], S0[::-1], sigma, rho)
        assert np.array_equal(rev[::-1], a), name
    # exact zeros
    m0, e0, S0 = (np.stack([case_moments("detuned", k)[i] for k in range(n)]) for i in range(3))
    L = _device_gains("kalman", bp, XO, UO, S0)
    z, st, _ = _predict(bp, XO, UO, KK, L, m0, e0, None, None, None)
    cov = z[:, :, np.r_[12:90, 92:95]]
    assert not st.any() and not cov.any() and not np.signbit(cov).any() and np.abs(z[:, :, 0:12]).max() > 0
    # the device's gains without a visit to the host
    measured = CASES["meas014"][0]
    Ld = batch.filter_gains_device(bp, XO, UO, S0, SIGMA, RHO, measured=measured)[0]
    dev, sd = batch.predict_covariance_lqg(bp, XO, UO, "device", KK=KK, mean0=m0, ehat0=e0, Sigma0=S0, sigma=SIGMA, rho=RHO,
                                           measured=measured)
    host, sh = batch.predict_covariance_lqg(bp, XO, UO, Ld, KK=KK, mean0=m0, ehat0=e0, Sigma0=S0, sigma=SIGMA, rho=RHO)
    assert np.array_equal(np.stack([p["raw"] for p in dev]), np.stack([p["raw"] for p in host])) and not sd.any() and not sh.any()
    assert np.isfinite(np.stack([p["raw"] for p in host])).all()


@gpu
def test_pred_is_fully_written():
    """the C call on a pred filled with NaN beforehand: no NaN is left"""
    import ctypes as C
    import torch
    from aircraftoptimalcontrol_amd import _lib, batch
    T, n = 17, 3
    XO, UO, KK, _ = windows(n, T)
    bp = _bp(XO)
    nominal = torch.from_numpy(batch.ensemble_nominal(XO, UO, KK)).to(bp.device)
    filt = torch.zeros((n, T, 36), dtype=torch.float64, device=bp.device)
    pred = torch.full((n, T, NREC), float("nan"), dtype=torch.float64, device=bp.device)
    nbytes = int(_lib.lib().aoc_track_covariance_lqg_scratch_bytes(n, T))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=bp.device)
    p = bp.c_problem(n)
    _lib.check(_lib.lib().aoc_track_covariance_lqg(C.byref(p), n, nominal.data_ptr(), filt.data_ptr(), None, None, None, None,
                                                   None, pred.data_ptr(), None, scratch.data_ptr(), nbytes))
    assert torch.isfinite(pred).all()


@gpu
def test_track_ensemble_adds_the_joint_prediction_and_keeps_every_other_bit():
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_ensemble import deltas
    T, B, mpo = 33, 130, 64
    XO, UO, KK, _ = windows(3, T)
    bp = _bp(XO)
    S0 = np.stack([case_moments("detuned", k)[2] for k in range(3)])
    kw = dict(delta=deltas(B), KK=KK, members_per_opt=mpo, sigma=SIGMA, seed=11, rho=RHO, trajectories=True, filter="device",
              Sigma0=S0, measured=(0, 1, 4))
    a = batch.track_ensemble(bp, XO, UO, **kw)
    b = batch.track_ensemble(bp, XO, UO, predict_joint=True, **kw)
    assert "predicted_joint" not in a and len(b["predicted_joint"]) == 3 and not b["predicted_joint_status"].any()
    for k in ("xx_reg", "uu_reg", "xhat", "dist", "meas", "stats", "est_stats", "status", "filter_status"):
        assert np.array_equal(a[k], b[k]), k
    grp = np.arange(B) // mpo                                  # the default mean0: of the deviations as the call forms them
    dx0 = (XO[grp, :, 0] + deltas(B)) - XO[grp, :, 0]
    m0 = np.stack([dx0[grp == k].mean(axis=0) for k in range(3)])
    pred, _ = batch.predict_covariance_lqg(bp, XO, UO, "device", KK=KK, mean0=m0, Sigma0=S0, sigma=SIGMA, rho=RHO,
                                           measured=(0, 1, 4))
    for k in range(3):
        assert np.array_equal(pred[k]["raw"], b["predicted_joint"][k]["raw"])


@gpu
@pytest.mark.parametrize("s", [0.1, 1.0])
def test_orthogonality_with_the_devices_own_kalman_gains(s):
    """The device's own Kalman gains (the same Sigma0, SIGMA, RHO; ehat0 = mean0): E_t is P^+_t of aoc_filter_gains' cov and
    C_t = E_t, each within 16x what the fp64 restatement shows on the same case (ORTH_E, ORTH_C)."""
    from aircraftoptimalcontrol_amd import batch
    g = _g4()[0]
    T = MC_T
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    S0 = np.diag((DELTA_SCALE * s) ** 2)
    bp = _problem(dict(g, xx_opt=xo))
    L, _, Pp, st = batch.filter_gains_device(bp, xo, uo, S0, SIGMA, RHO)
    pred, status = batch.predict_covariance_lqg(bp, xo, uo, L[0], KK=KK, Sigma0=S0, sigma=SIGMA, rho=RHO)
    ge, gc = orthogonality_gap(s, got=pred[0]["raw"], P_post=Pp[0])
    print("s = %g: E against P+ %.3g (bound %.3g), C against E %.3g (bound %.3g)" % (s, ge, 16 * ORTH_E[s], gc, 16 * ORTH_C[s]))
    assert not st.any() and not status.any()
    assert ge <= 16 * ORTH_E[s] and gc <= 16 * ORTH_C[s], (ge, gc)


@gpu
def test_zero_gains_and_no_measurement_noise_is_the_uncontrolled_recursion():
    """L = 0, rho = 0: the estimate never moves, so X follows X' = A X A^T + W of a loop without feedback — the covariance of
    aoc_track_covariance with zero tracking gains — to the rounding of the cancellation, 16 REF_GAP in the dX metric."""
    from aircraftoptimalcontrol_amd import batch
    T, n = 33, 3
    XO, UO, KK, _ = windows(n, T)
    bp = _bp(XO)
    m0, S0 = start_moments(n)
    got, st, pred = _predict(bp, XO, UO, KK, np.zeros((n, 6, 6, T)), m0, None, S0, SIGMA, None)
    free, sf = batch.predict_covariance(bp, XO, UO, KK=np.zeros_like(KK), mean0=m0, Sigma0=S0, sigma=SIGMA)
    assert not st.any() and not sf.any()
    for k in range(n):
        want = free[k]["cov_dx"]
        d = np.sqrt(np.einsum("iit->it", want).max(axis=1))
        gap = (np.abs(pred[k]["cov_dx"] - want).max(axis=2) / np.outer(d, d)).max()
        print("optimum %d: X against A X A^T + W: %.3g (bound %.3g)" % (k, gap, TOL))
        assert gap <= TOL
        assert np.array_equal(pred[k]["cov_e"][:, :, 0], S0[k]) and np.array_equal(pred[k]["cov_dx_e"][:, :, 0], S0[k])


@gpu
def test_a_bad_optimum_among_good_ones():
    """Optimum 1 of 3 has a NaN in its L, optimum 2's copy in a second call V_opt <= 0 mid-way: status says so, the
    neighbours' records are bit-identical to a clean call, nothing faults."""
    T = 40
    XO, UO, KK, _ = windows(3, T)
    bp = _bp(XO)
    m0, S0 = start_moments(3)
    L = _device_gains("kalman", bp, XO, UO, S0)
    clean, st0, _ = _predict(bp, XO, UO, KK, L, m0, None, S0, SIGMA, RHO)
    assert not st0.any()
    Lb = L.copy()
    Lb[1, 2, 3, 20] = np.nan
    got, st, _ = _predict(bp, XO, UO, KK, Lb, m0, None, S0, SIGMA, RHO)
    assert st[1] & ST_NAN and st[0] == 0 and st[2] == 0
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    assert np.array_equal(got[1, :20], clean[1, :20]) and np.isnan(got[1, 20:, 33:54]).any()
    bad = XO.copy()
    bad[2, 2, 20] = -3.0
    got, st, _ = _predict(bp, bad, UO, KK, L, m0, None, S0, SIGMA, RHO)
    assert st[2] & ST_VNONPOS and st[0] == 0 and st[1] == 0
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    assert np.array_equal(got[2, :20], clean[2, :20])


@gpu
@pytest.mark.parametrize("s", [0.1, 1.0])
def test_prediction_against_the_devices_own_monte_carlo(s):
    """The LQG ensemble of test_gpu_lqg.py's Monte Carlo (2048 members, the first 200 samples of g4, SIGMA, RHO, MC_SEED,
    mc_members(s), mc_gains(s)) against predict_covariance_lqg: at s = 0.1 every z <= 5, at s = 1.0 the covariance of dx
    disagrees, z_cov >= 15 — the conditions the CPU checker meets alone (tests/test_lqgcov_abi.py)."""
    from aircraftoptimalcontrol_amd import batch
    g = _g4()[0]
    xo, uo, KK, L, _ = mc_gains(s)
    d, m0, S0 = mc_members(s)
    bp = _problem(dict(g, xx_opt=xo))
    r = batch.track_ensemble(bp, xo, uo, delta=d, KK=KK, sigma=SIGMA, seed=MC_SEED, filter=L, rho=RHO, trajectories=True,
                             predict_joint=True, mean0=m0, Sigma0=S0)
    assert not r["status"].any() and not r["predicted_joint_status"].any()
    dx = r["xx_reg"] - xo[None]
    err = dx - (r["xhat"] - xo[None])
    du = (r["uu_reg"] - uo[None])[:, :, :MC_T - 1]
    z = joint_z(dx, err, du, r["predicted_joint"][0])
    print("s = %g: %s" % (s, z))
    if s == 0.1:
        assert max(max(z["dx"]), max(z["e"]), max(z["du"]), z["cross"]) <= 5, z
    else:
        assert z["dx"][0] >= 15, z


@gpu
def test_example_saves_the_joint_prediction(tmp_path):
    """examples/run_tracking_ensemble.py --rho ... --predict-joint FILE.npz as a process: one JSON line with the predicted RMS
    of dx and of e beside the sampled ones, and a file whose arrays have the stated shapes."""
    import json
    from test_gpu_drivers import _run as run_example
    g, _, T = _g4()
    np.save(tmp_path / "xx_star.npy", g["xx_opt"])
    np.save(tmp_path / "uu_star.npy", g["uu_opt"])
    out = run_example("run_tracking_ensemble.py", "--data", tmp_path, "--members", 256, "--seed", 5, "--dt", float(g["dt"]),
                      "--sigma", *SIGMA, "--delta", *(0.1 * DELTA_SCALE), "--rho", *RHO, "--predict-joint", tmp_path / "joint.npz")
    lines = [l for l in out.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for key in ("predicted_rms_dx", "predicted_rms_estimation_error", "rms_dx", "rms_estimation_error"):
        assert len(line[key]) == 6 and np.isfinite(line[key]).all(), key
    # the prediction is of the size of what was sampled (256 members, linear regime)
    assert np.allclose(line["predicted_rms_estimation_error"], line["rms_estimation_error"], rtol=0.25)
    f = np.load(tmp_path / "joint.npz")
    shapes = dict(mean_dx=(6, T), cov_dx=(6, 6, T), mean_e=(6, T), cov_e=(6, 6, T), cov_dx_e=(6, 6, T), cov_xhat=(6, 6, T),
                  mean_du=(2, T), cov_du=(2, 2, T), status=())
    for k, sh in shapes.items():
        assert f[k].shape == sh, (k, f[k].shape)
    assert int(f["status"]) == 0
