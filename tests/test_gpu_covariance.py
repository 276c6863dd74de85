"""aoc_track_covariance / batch.predict_covariance: what linear theory predicts for a closed-loop tracking ensemble.

The checker is numpy_covariance below: the recursion of include/aoc.h in NumPy fp64 with A, B and the stepped state from
the oracle's Dynamics.step (tests/test_covariance_abi.py checks it without a GPU, against a Monte Carlo of the oracle's own
closed loop).  The device differs from it in the order of the sums, in fused multiply-adds and in its own sin / cos /
reciprocal inside the Jacobians, so the bar is not bit-identity but a multiple of the checker's OWN rounding: the largest
scaled gap between the checker in fp64 and the same checker in np.longdouble over the cases of test_parity_with_the_checker
(REF_GAP, measured on the CPU by reference_gap below), times 16."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as orc
from test_gpu_ensemble import DELTA_SCALE, SIGMA, _g4, _problem, host_loop  # noqa: F401

pytestmark = pytest.mark.gpu

TRI = [(i, j) for i in range(6) for j in range(i, 6)]
ST_NAN, ST_VNONPOS = 1, 2
# the largest scaled gap (metric: scaled_gap below) between numpy_covariance in fp64 and in np.longdouble over every case
# of test_parity_with_the_checker, measured: 2.14e-14 (1.1e-14 on T = 200, n_opt = 3 alone); the device may be 16x that
REF_GAP = 2.14e-14
TOL = 16 * REF_GAP
SIZES_T = (3, 17, 33, 200)
SIZES_N = (1, 3, 70)
# the horizon edges, run at n_opt = 3 alone: T - 1 = 15 and 31 are the last record of a block of the 16-record prefetch (the
# block behind it holds nothing), T = 18 puts one stage into the second block, T = 4 is the first horizon with an inner stage
EDGE_T = (4, 16, 18, 32)
EDGE_N = 3


def jacobians(mdl, xo, uo):
    """A (T-1,6,6), B (T-1,6,2), stepped state (T-1,6) of the oracle's Dynamics.step along (xo (6,T), uo (2,T))"""
    T = xo.shape[1]
    A, B, xp = np.zeros((T - 1, 6, 6)), np.zeros((T - 1, 6, 2)), np.zeros((T - 1, 6))
    for t in range(T - 1):
        x1, fx, fu = orc.step(mdl, xo[:, t], uo[:, t])[:3]
        A[t], B[t], xp[t] = np.asarray(fx).reshape(6, 6).T, np.asarray(fu).reshape(2, 6).T, x1
    return A, B, xp


def numpy_covariance(jac, xo, KK, mean0=None, Sigma0=None, sigma=None, dtype=np.float64):
    """The recursion of include/aoc.h for ONE optimum: jac = jacobians(...), xo (6,T), KK (2,6,T), mean0 (6,), Sigma0 (6,6),
    sigma (6,) (None = 0 each) -> records (T,32) in `dtype`."""
    A, B, xp = (a.astype(dtype) for a in jac)
    T = xo.shape[1]
    K = np.asarray(KK).astype(dtype)
    m = np.zeros(6, dtype) if mean0 is None else np.asarray(mean0).astype(dtype)
    P = np.zeros((6, 6), dtype) if Sigma0 is None else np.asarray(Sigma0).astype(dtype)
    W = np.zeros((6, 6), dtype) if sigma is None else np.diag(np.asarray(sigma).astype(dtype) ** 2)
    rec = np.zeros((T, 32), dtype)
    for t in range(T):
        rec[t, 0:6] = m
        rec[t, 6:27] = [P[i, j] for i, j in TRI]
        if t == T - 1:
            break
        Kt = K[:, :, t]
        rec[t, 27:29] = Kt @ m
        KPK = Kt @ P @ Kt.T
        rec[t, 29:32] = KPK[0, 0], KPK[0, 1], KPK[1, 1]
        F = A[t] + B[t] @ Kt
        c = xp[t] - xo[:, t + 1].astype(dtype)
        m = F @ m + c
        P = F @ P @ F.T + W
        P = (P + P.T) / 2
    return rec


def scaled_gap(got, want):
    """The largest gap between two arrays of records (..., T, 32) in the metric of the issue: entry (i,j) of P over
    s_i s_j, s_i = max_t sqrt(P_ii) of `want`; m_i over max(s_i, max_t |m_i|); the input moments likewise.  An entry whose
    scale is 0 must agree exactly (its gap is then 0, else inf)."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    w64 = np.asarray(want, dtype=np.float64)
    diag = [6 + TRI.index((i, i)) for i in range(6)]
    s = np.sqrt(np.abs(w64[..., diag]).max(axis=-2))                                   # (..., 6)
    su = np.sqrt(np.abs(w64[..., [29, 31]]).max(axis=-2))                              # (..., 2)
    scale = np.empty(w64.shape[:-2] + (32,))
    scale[..., 0:6] = np.maximum(s, np.abs(w64[..., 0:6]).max(axis=-2))
    scale[..., 6:27] = np.stack([s[..., i] * s[..., j] for i, j in TRI], axis=-1)
    scale[..., 27:29] = np.maximum(su, np.abs(w64[..., 27:29]).max(axis=-2))
    scale[..., 29:32] = np.stack([su[..., 0] ** 2, su[..., 0] * su[..., 1], su[..., 1] ** 2], axis=-1)
    d = np.abs(got - want).max(axis=-2).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(scale > 0, d / scale, np.where(d == 0, 0.0, np.inf))
    return float(g.max())


_CACHE = {}


def g4_jacobians():
    """g4's optimum with its Jacobians along the whole horizon, computed once: windows are cuts of it"""
    if "g4" not in _CACHE:
        g, mdl, _ = _g4()
        _CACHE["g4"] = (g, mdl, jacobians(mdl, g["xx_opt"], g["uu_opt"]))
    return _CACHE["g4"]


def windows(n_opt, T):
    """n_opt windows of g4 at offsets 5k: XO (n,6,T), UO (n,2,T), KK (n,2,6,T) (the reference's gains, cut) and per window
    the Jacobians"""
    g, _, (A, B, xp) = g4_jacobians()
    off = [5 * k for k in range(n_opt)]
    XO = np.stack([g["xx_opt"][:, o:o + T] for o in off])
    UO = np.stack([g["uu_opt"][:, o:o + T] for o in off])
    KK = np.stack([g["KK"][:, :, o:o + T] for o in off])
    jac = [(A[o:o + T - 1], B[o:o + T - 1], xp[o:o + T - 1]) for o in off]
    return XO, UO, KK, jac


def start_moments(n_opt, seed=5):
    """mean0 (n,6) and a full symmetric positive Sigma0 (n,6,6) of the size of the ensemble tests' spread"""
    rng = np.random.default_rng(seed)
    m0 = rng.normal(size=(n_opt, 6)) * DELTA_SCALE * 0.1
    L = rng.normal(size=(n_opt, 6, 6)) * (DELTA_SCALE * 0.1)[None, :, None] / np.sqrt(6)
    S0 = L @ L.transpose(0, 2, 1)
    return m0, (S0 + S0.transpose(0, 2, 1)) / 2


CASES = {"plain": (False, False), "noise": (True, False), "moments": (False, True), "noise_moments": (True, True)}


def case_args(name, n_opt):
    noise, mom = CASES[name]
    m0, S0 = start_moments(n_opt) if mom else (None, None)
    return m0, S0, (SIGMA if noise else None)


def checker_records(jac, XO, KK, m0, S0, sigma, dtype=np.float64):
    return np.stack([numpy_covariance(jac[k], XO[k], KK[k], None if m0 is None else m0[k], None if S0 is None else S0[k],
                                      sigma, dtype) for k in range(len(jac))])


def reference_gap(sizes_T=SIZES_T, sizes_n=SIZES_N):
    """The checker's own rounding: the largest scaled gap between numpy_covariance in fp64 and in np.longdouble over the
    cases of test_parity_with_the_checker, test_parity_at_the_horizon_edges and test_a_nominal_that_is_not_a_rollout.  Needs
    no GPU."""
    worst = 0.0
    for T, n_opt in [(T, n) for T in sizes_T for n in sizes_n] + [(T, EDGE_N) for T in EDGE_T]:
        XO, _, KK, jac = windows(n_opt, T)
        for name in CASES:
            m0, S0, sigma = case_args(name, n_opt)
            worst = max(worst, scaled_gap(checker_records(jac, XO, KK, m0, S0, sigma),
                                          checker_records(jac, XO, KK, m0, S0, sigma, np.longdouble)))
    xo, _, KK, jac = offset_nominal(33)
    for name in ("plain", "noise_moments"):
        m0, S0, sigma = case_args(name, 1)
        worst = max(worst, scaled_gap(checker_records([jac], xo[None], KK[None], m0, S0, sigma),
                                      checker_records([jac], xo[None], KK[None], m0, S0, sigma, np.longdouble)))
    return worst


def offset_nominal(T):
    """g4's states plus a smooth offset: NOT a rollout, so c_t != 0"""
    g, mdl, _ = _g4()
    tt = np.arange(T) / 200.0
    xo = g["xx_opt"][:, :T] + np.outer(DELTA_SCALE * 0.01, np.sin(2 * np.pi * tt) + 0.5 * tt)
    uo = g["uu_opt"][:, :T]
    return xo, uo, g["KK"][:, :, :T], jacobians(mdl, xo, uo)


def _predict_on(bp, XO, UO, KK, m0, S0, sigma):
    from aircraftoptimalcontrol_amd import batch
    pred, status = batch.predict_covariance(bp, XO, UO, KK=KK, mean0=m0, Sigma0=S0, sigma=sigma)
    return np.stack([p["raw"] for p in pred]), status, pred


def _predict(g, XO, UO, KK, m0, S0, sigma):
    return _predict_on(_problem(dict(g, xx_opt=XO[0])), XO, UO, KK, m0, S0, sigma)


@pytest.mark.parametrize("n_opt", SIZES_N)
@pytest.mark.parametrize("T", SIZES_T)
def test_parity_with_the_checker(T, n_opt):
    """Windows of g4 at offsets 5k; T = 3 is the shortest horizon the call takes, 17 and 33 end one sample behind a block of
    the 16-record prefetch, 70 optima are more wavefronts than one; with and without noise, with and without mean0 / Sigma0."""
    _parity(T, n_opt)


@pytest.mark.parametrize("T", EDGE_T)
def test_parity_at_the_horizon_edges(T):
    """The parity test at the horizons EDGE_T (see there) with three optima."""
    _parity(T, EDGE_N)


def _parity(T, n_opt):
    g = g4_jacobians()[0]
    XO, UO, KK, jac = windows(n_opt, T)
    for name in CASES:
        m0, S0, sigma = case_args(name, n_opt)
        want = checker_records(jac, XO, KK, m0, S0, sigma)
        got, status, pred = _predict(g, XO, UO, KK, m0, S0, sigma)
        gap = scaled_gap(got, want)
        print("T = %d, n_opt = %d, %s: scaled gap %.3g (bound %.3g)" % (T, n_opt, name, gap, TOL))
        assert got.shape == (n_opt, T, 32) and not status.any()
        assert gap <= TOL, (T, n_opt, name, gap)
        assert np.array_equal(got[:, T - 1, 27:], np.zeros((n_opt, 5))) and not np.signbit(got[:, T - 1, 27:]).any()
    # the unpacked form is the record
    from aircraftoptimalcontrol_amd import batch
    mean_dx, cov_dx, mean_du, cov_du = batch.covariance_moments(got[0])
    assert np.array_equal(pred[0]["cov_dx"], cov_dx) and np.array_equal(cov_dx, cov_dx.transpose(1, 0, 2))
    assert np.array_equal(mean_dx, got[0, :, 0:6].T) and np.array_equal(cov_du[0, 1], got[0, :, 30])


def test_a_nominal_that_is_not_a_rollout():
    """c_t != 0: the mean moves although mean0 = 0"""
    g = g4_jacobians()[0]
    T = 33
    xo, uo, KK, jac = offset_nominal(T)
    assert np.abs(jac[2] - xo[:, 1:].T).max() > 1e-6
    for name in ("plain", "noise_moments"):
        m0, S0, sigma = case_args(name, 1)
        want = checker_records([jac], xo[None], KK[None], m0, S0, sigma)
        got, status, _ = _predict(g, xo[None], uo[None], KK[None], m0, S0, sigma)
        gap = scaled_gap(got, want)
        print("offset nominal, %s: scaled gap %.3g (bound %.3g)" % (name, gap, TOL))
        assert gap <= TOL and not status.any()
        assert np.abs(got[0, 1:, 0:6]).max() > 1e-6
        if name == "plain":   # the defect itself is the plant's own arithmetic: exact
            assert np.array_equal(got[0, 1, 0:6], jac[2][0] - xo[:, 1])


G13_K_SEED = 13
G13_BOUND = 1e-12      # the gate of tests/test_gpu_parity.py test_step_batch_wide_angles_vs_golden on the same Jacobians


def g13_optima(K=None):
    """Three-sample optima on ALL the points of tests/golden/g13_step_wide.npz (216: angles over +-4 pi, up to 2^24, V from
    0.05 to 300) at its dt: optimum i has x_opt_0 = x[i], u_0 = u_1 = u[i], x_opt_1 = x_opt_2 = xp[i] widened to fp64, and
    the gains K (2,6) at every sample (None = 0).  The device's step is xp bit for bit (test_step_batch_wide_angles_vs_golden),
    so c_0 = +0.0.  -> g, XO (n,6,3), UO (n,2,3), KK (n,2,6,3), A (n,6,6) and B (n,6,2) of stage 0 from the golden fx = A^T,
    fu = B^T."""
    g = load_golden("g13_step_wide")
    xp = g["xp"].astype(np.float64)
    n = xp.shape[0]
    XO = np.stack([g["x"], xp, xp], axis=2)
    UO = np.stack([g["u"]] * 3, axis=2)
    KK = np.zeros((n, 2, 6, 3)) if K is None else np.broadcast_to(np.asarray(K)[None, :, :, None], (n, 2, 6, 3)).copy()
    return g, XO, UO, KK, g["fx"].transpose(0, 2, 1), g["fu"].transpose(0, 2, 1)


def g13_gains():
    """the fixed gains of order one of the G13 tests, the same at every point"""
    return np.random.default_rng(G13_K_SEED).normal(size=(2, 6))


def g13_problem(g):
    from aircraftoptimalcontrol_amd import batch
    return batch.BatchProblem(np.eye(6), np.eye(2), np.eye(6), np.zeros((6, 3)), np.zeros((2, 3)), float(g["dt"]))


def g13_gap(got, A, B, K=None):
    """got (n,6,6) against A + B K formed in np.longdouble, per entry over |A_ij| + sum_r |B_ir K_rj| -> (the largest gap
    over the entries whose scale is not 0, the point that sets it, its entry); an entry whose scale is 0 must be exactly
    zero in `got` (asserted here: the sparsity of A and B)."""
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    Kl = np.zeros((2, 6), np.longdouble) if K is None else np.asarray(K).astype(np.longdouble)
    want = Al + np.einsum("nir,rj->nij", Bl, Kl)
    scale = (np.abs(Al) + np.einsum("nir,rj->nij", np.abs(Bl), np.abs(Kl))).astype(np.float64)
    live = scale > 0
    assert got.shape == scale.shape and not got[~live].any(), "an entry outside the sparsity of A + B K is not zero"
    gap = np.zeros(scale.shape)
    gap[live] = (np.abs(got.astype(np.longdouble) - want)[live]).astype(np.float64) / scale[live]
    n, i, j = np.unravel_index(int(np.argmax(gap)), gap.shape)
    return float(gap[n, i, j]), int(n), (int(i), int(j))


def g13_report(what, gap, point, entry, g):
    """print the largest gap and the point that sets it -> the record of it for AOC_TEST_RECORDS"""
    x = g["x"][point]
    print("%s: largest gap %.3g (bound %.3g) at point %d, entry %s: V = %.4g, theta = %.9g, gamma = %.9g"
          % (what, gap, G13_BOUND, point, entry, x[2], x[3], x[5]))
    return dict(what=what, gap=gap, bound=G13_BOUND, point=point, entry=list(entry), V=float(x[2]), theta=float(x[3]),
                gamma=float(x[5]))


@pytest.mark.parametrize("gains", [False, True], ids=["K0", "K13"])
def test_stage_records_at_wide_angles(gains):
    """k_cov_stage<true> off the g4 fixture, read through aoc_track_covariance alone: three-sample optima on all 216 points of
    G13 (g13_optima), mean0 = e_j, no Sigma0, no noise, so the record of sample 1 holds m_1 = F[:, j] — one product with 1.0
    and sums with +0.0: the device's own entry, unrounded.  With K = 0 that is A, with the seeded K of order one A + B K; both
    against the golden fx, fu in np.longdouble, per entry over |A_ij| + sum_r |B_ir K_rj|, bound 1e-12 (the gate those
    Jacobians already meet at aoc_step_batch); every entry outside the sparsity of A + B K is exactly zero.  status is
    AOC_ST_VNONPOS exactly on the 30 optima whose xp[i, 2] <= 0 (stage 1 starts from V <= 0; their sample-1 record comes
    from stage 0 and is compared like the rest).
    Measured on an MI355X: K = 0: 3.92e-13; seeded K: 3.49e-13; both at entry (2, 2) of point 133, the cancelling entry that
    sets the 3.9e-13 of aoc_step_batch; the parity gaps at EDGE_T stay below 3.0e-15."""
    from test_gpu_parity import _record
    K = g13_gains() if gains else None
    g, XO, UO, KK, A, B = g13_optima(K)
    n = XO.shape[0]
    bp = g13_problem(g)
    assert n == 216 and int((XO[:, 2, 1] <= 0).sum()) == 30
    F = np.zeros((n, 6, 6))
    for j in range(6):
        got, status, _ = _predict_on(bp, XO, UO, KK, np.eye(6)[j], None, None)
        F[:, :, j] = got[:, 1, 0:6]
        assert np.array_equal(got[:, 0, 0:6], np.broadcast_to(np.eye(6)[j], (n, 6)))
        assert np.array_equal(status, np.where(XO[:, 2, 1] <= 0, ST_VNONPOS, 0)), j
    gap, point, entry = g13_gap(F, A, B, K)
    rec = g13_report("F = A%s through aoc_track_covariance" % (" + B K" if gains else ""), gap, point, entry, g)
    _record("g13_cov_stage_%s.json" % ("K13" if gains else "K0"), dict(points=n, **rec))
    assert gap <= G13_BOUND, (gap, point, entry)


def test_the_defect_at_wide_angles():
    """mean0 = 0 and x_opt_1 moved off the rollout by DELTA_SCALE * 0.01 on all 216 points of G13: m_1 = c_0 = xp - x_opt_1
    is the plant's own arithmetic, so it equals the host's fp64 difference bit for bit (the assertion of
    test_a_nominal_that_is_not_a_rollout on g4), whatever the gains."""
    g, XO, UO, KK, _, _ = g13_optima(g13_gains())
    xp = XO[:, :, 2].copy()
    XO[:, :, 1] = xp + DELTA_SCALE * 0.01
    got, status, _ = _predict_on(g13_problem(g), XO, UO, KK, None, None, None)
    assert np.array_equal(got[:, 1, 0:6], xp - XO[:, :, 1]) and np.abs(got[:, 1, 0:6]).max() > 1e-3
    assert not got[:, 0, 0:6].any()
    assert np.array_equal(status, np.where(XO[:, 2, 1] <= 0, ST_VNONPOS, 0))


def test_exact_cases():
    """No Sigma0, no noise: every covariance entry is +0.0; the same call again gives the same bits; optimum k of a
    70-optimum call has the bits of the same optimum called alone."""
    g = g4_jacobians()[0]
    T = 33
    XO, UO, KK, _ = windows(70, T)
    m0, _ = start_moments(70)
    got, status, _ = _predict(g, XO, UO, KK, m0, None, None)
    cov = got[:, :, np.r_[6:27, 29:32]]
    assert not cov.any() and not np.signbit(cov).any() and np.abs(got[:, :, 0:6]).max() > 0
    m0, S0 = start_moments(70)
    a, _, _ = _predict(g, XO, UO, KK, m0, S0, SIGMA)
    b, _, _ = _predict(g, XO, UO, KK, m0, S0, SIGMA)
    assert np.array_equal(a, b)
    for k in (0, 1, 37, 69):
        one, _, _ = _predict(g, XO[k:k + 1], UO[k:k + 1], KK[k:k + 1], m0[k:k + 1], S0[k:k + 1], SIGMA)
        assert np.array_equal(one[0], a[k]), k


def test_a_bad_optimum_among_good_ones():
    """Optimum 1 of 3 has V_opt <= 0 mid-way, optimum 2's copy in a second call a NaN gain: status says so, the neighbours'
    records are bit-identical to a call without it, nothing faults."""
    g = g4_jacobians()[0]
    T = 40
    XO, UO, KK, _ = windows(3, T)
    m0, S0 = start_moments(3)
    clean, st0, _ = _predict(g, XO, UO, KK, m0, S0, SIGMA)
    assert not st0.any()
    bad = XO.copy()
    bad[1, 2, 20] = -3.0
    got, st, _ = _predict(g, bad, UO, KK, m0, S0, SIGMA)
    assert st[1] & ST_VNONPOS and st[0] == 0 and st[2] == 0
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    assert np.array_equal(got[1, :20], clean[1, :20])
    Kb = KK.copy()
    Kb[2, 1, 3, 7] = np.nan
    got, st, _ = _predict(g, XO, UO, Kb, m0, S0, SIGMA)
    assert st[2] & ST_NAN and st[0] == 0 and st[1] == 0
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    # V_opt <= 0 at the LAST sample is no stage's business
    last = XO.copy()
    last[0, 2, T - 1] = -1.0
    _, st, _ = _predict(g, last, UO, KK, m0, S0, SIGMA)
    assert not st.any()


def z_scores(S, mean, P, m, M):
    """z_cov = max |S_ij - P_ij| / sqrt((P_ii P_jj + P_ij^2) / M), z_mean = max |mean_i - m_i| / sqrt(P_ii / M) over the
    samples and entries; S, P (6,6,T), mean, m (6,T)"""
    d = np.einsum("iit->it", P)
    with np.errstate(divide="ignore", invalid="ignore"):
        zc = np.abs(S - P) / np.sqrt((d[:, None, :] * d[None, :, :] + P ** 2) / M)
        zm = np.abs(mean - m) / np.sqrt(d / M)
    return float(np.nanmax(zc)), float(np.nanmax(zm))


MC_T, MC_M, MC_SEED = 200, 2048, 7


def mc_members(s, M=MC_M):
    """deltas of the Monte Carlo of the issue and the POPULATION moments they are drawn from"""
    d = np.random.default_rng(3).normal(size=(M, 6)) * DELTA_SCALE * s
    return d, np.zeros(6), np.diag((DELTA_SCALE * s) ** 2)


@pytest.mark.parametrize("s", [0.1, 1.0])
def test_prediction_against_the_devices_own_monte_carlo(s):
    """2048 members, T = 200, sigma = SIGMA: at s = 0.1 the sampled moments agree with the prediction within sampling error
    (both z <= 5), at s = 1.0 the covariance does not (z_cov >= 15): the conditions the CPU reference meets alone
    (tests/test_covariance_abi.py)."""
    from aircraftoptimalcontrol_amd import batch
    g, _, _ = _g4()
    T = MC_T
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    d, m0, S0 = mc_members(s)
    r = batch.track_ensemble(_problem(dict(g, xx_opt=xo)), xo, uo, delta=d, KK=KK, sigma=SIGMA, seed=MC_SEED, envelope=True,
                             predict=True, mean0=m0, Sigma0=S0)
    n, mean, S = batch.envelope_moments(r["envelope"][0]["raw"])
    assert (n == MC_M).all() and not r["predicted_status"].any()
    p = r["predicted"][0]
    zc, zm = z_scores(S, mean, p["cov_dx"], p["mean_dx"], MC_M)
    print("s = %g: z_cov = %.2f, z_mean = %.2f" % (s, zc, zm))
    if s == 0.1:
        assert zc <= 5 and zm <= 5, (zc, zm)
    else:
        assert zc >= 15, zc


def test_one_pass_quantiles():
    """quantiles= with bins="predicted" at s = 0.1: no envelope call; the counts are NumPy's binning of the device's own
    trajectories under the same bins; at k = 6 the two end bins together hold at most 1 % of any (sample, channel); the
    tubes agree with the two-pass route's within the sum of the two bin widths."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_histogram import Q3, _check, _hist
    g, _, _ = _g4()
    T = MC_T
    xo, uo, KK = g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]
    d, m0, S0 = mc_members(0.1)
    bp = _problem(dict(g, xx_opt=xo))
    kw = dict(delta=d, KK=KK, sigma=SIGMA, seed=MC_SEED)
    r = batch.track_ensemble(bp, xo, uo, quantiles=Q3, bins="predicted", mean0=m0, Sigma0=S0, **kw)
    assert "envelope" not in r and "predicted" in r
    assert np.array_equal(np.stack(r["bins"]), batch.histogram_bins_predicted(r["predicted"][0]["raw"], 6.0))
    old = batch.track_ensemble(bp, xo, uo, trajectories=True, **kw)
    for k in ("stats", "status", "first_bad"):
        assert np.array_equal(r[k], old[k]), k
    _check(r, old, xo, uo, T, "predicted bins")
    h = _hist(r)[0]                                                                    # (T,8,64)
    ends = (h[:, :, 0] + h[:, :, 63]) / np.maximum(h.sum(axis=-1), 1)
    print("largest share of the two end bins: %.4f" % ends.max())
    assert ends.max() <= 0.01
    two = batch.track_ensemble(bp, xo, uo, quantiles=Q3, **kw)
    assert "envelope" in two
    gap = np.abs(r["tube"][0] - two["tube"][0])
    lim = (r["tube_width"][0] + two["tube_width"][0])[None]
    live = np.isfinite(two["tube"][0])
    assert np.array_equal(live, np.isfinite(r["tube"][0])) and (gap[live] <= np.broadcast_to(lim, gap.shape)[live]).all()



def test_predict_defaults_and_the_other_outputs_keep_their_bits():
    """Two nominals, B = 322 in groups of 192: predict=True without moments takes the population mean and covariance of
    each group's own initial deviations, returns what predict_covariance returns for them, and changes no other output."""
    from aircraftoptimalcontrol_amd import batch
    from test_gpu_ensemble import _two_nominals, deltas
    g, _, _ = _g4()
    T, B, mpo = 33, 322, 192
    XO, UO = _two_nominals(g)
    XO, UO = XO[:, :, :T], UO[:, :, :T]
    KK = np.stack([g["KK"][:, :, :T]] * 2)
    bp = _problem(dict(g, xx_opt=XO[0]))
    kw = dict(delta=deltas(B), KK=KK, members_per_opt=mpo, sigma=SIGMA, seed=11)
    r = batch.track_ensemble(bp, XO, UO, envelope=True, predict=True, **kw)
    old = batch.track_ensemble(bp, XO, UO, envelope=True, **kw)
    assert sorted(set(r) - set(old)) == ["predicted", "predicted_status"] and not r["predicted_status"].any()
    for k in ("stats", "status", "group"):
        assert np.array_equal(r[k], old[k]), k
    assert all(np.array_equal(a["raw"], b["raw"]) for a, b in zip(r["envelope"], old["envelope"]))
    d = kw["delta"]
    dx0 = [(XO[k, :, 0] + d[k * mpo:(k + 1) * mpo]) - XO[k, :, 0] for k in range(2)]
    m0 = np.stack([v.mean(axis=0) for v in dx0])
    S0 = np.stack([np.cov(v.T, bias=True) for v in dx0])
    S0 = 0.5 * (S0 + S0.transpose(0, 2, 1))
    want, _ = batch.predict_covariance(bp, XO, UO, KK=KK, mean0=m0, Sigma0=S0, sigma=SIGMA)
    for k in range(2):
        assert np.array_equal(r["predicted"][k]["raw"], want[k]["raw"]), k
        # sample 0 of the prediction IS the sampled moment of sample 0 (the envelope's, to its own rounding)
        n, mean, cov = batch.envelope_moments(r["envelope"][k]["raw"])
        assert np.allclose(r["predicted"][k]["mean_dx"][:, 0], mean[:, 0], rtol=0, atol=1e-12)
        assert np.allclose(r["predicted"][k]["cov_dx"][:, :, 0], cov[:, :, 0], rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="symmetric"):
        batch.predict_covariance(bp, XO, UO, KK=KK, Sigma0=np.triu(np.ones((6, 6))))
    with pytest.raises(ValueError, match="predicted"):
        batch.track_ensemble(bp, XO, UO, bins="predicted", **kw)


def test_example_saves_the_prediction(tmp_path):
    """examples/run_tracking_ensemble.py --predict FILE.npz as a process: the file's arrays equal batch.predict_covariance
    from the population moments of the example's perturbation, and the JSON line names the file."""
    import json
    from test_gpu_drivers import _run
    from aircraftoptimalcontrol_amd import batch, problems
    g, _, T = _g4()
    np.save(tmp_path / "xx_star.npy", g["xx_opt"])
    np.save(tmp_path / "uu_star.npy", g["uu_opt"])
    f = tmp_path / "pred.npz"
    out = _run("run_tracking_ensemble.py", "--data", tmp_path, "--members", 256, "--seed", 5, "--dt", float(g["dt"]),
               "--sigma", *SIGMA, "--predict", f)
    line = json.loads(out.strip().split("\n")[-1])
    Q, R, QT = problems.tracking_weights()
    bp = batch.BatchProblem(Q, R, QT, np.zeros((6, T)), np.zeros((2, T)), float(g["dt"]))
    want, _ = batch.predict_covariance(bp, g["xx_opt"], g["uu_opt"], mean0=np.zeros(6), Sigma0=np.diag(DELTA_SCALE ** 2),
                                       sigma=SIGMA)
    saved = dict(np.load(f, allow_pickle=False))
    assert sorted(saved) == ["cov_du", "cov_dx", "mean_du", "mean_dx", "raw"]
    for k, v in want[0].items():
        assert np.array_equal(saved[k], v), k
    assert saved["raw"].shape == (T, 32) and line["predict"]["file"] == str(f) and line["members"] == 256
    assert np.array_equal(line["predict"]["max_std"], np.sqrt(np.einsum("iit->it", want[0]["cov_dx"])).max(axis=1))
