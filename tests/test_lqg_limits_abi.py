"""CPU-side checks of aoc_track_ensemble_lqg_limited (actuator limits in the loop of the estimator): the symbols bind and the
ABI revision is what it was, the scratch query, every refusal with its reason and in its order, the keyword rules of
batch.track_ensemble(filter=, u_min= / u_max= / u_rate=, est_input=), and the host checker of tests/test_gpu_lqg_limits.py —
lqg_loop_limited below: lqg_loop of tests/test_gpu_lqg.py with the selection of host_loop_limited (tests/test_limits_abi.py)
between forming the demand and stepping the plant, and with the estimator's correction B_t (u_t - v_t) of include/aoc.h.

What the checker is held to without a GPU: with infinite limits it is lqg_loop bit for bit; on a LINEAR plant the informed
estimator's error under limits is that of the loop without limits; its own rounding (REF_GAP_LIM, fp64 against np.longdouble
in the estimator and the correction) over the cases of the GPU parity tests; the conditions under which those tests may
compare the cut statistics exactly; and the Monte Carlo of the loop under limits against the filter's own covariance."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from aircraftoptimalcontrol_amd import _lib
from test_limits_abi import INF2, U_MAX, U_MIN, U_RATE

REC = 56 * 8   # bytes of scratch per (optimum, sample)
EST_INPUTS = ("applied", "demanded")
# the largest scaled gap (scaled_gap of tests/test_gpu_lqg.py) between lqg_loop_limited in fp64 and with the estimator and
# the correction in np.longdouble over every case of the GPU parity tests (PARITY_RUNS x CASES x EST_INPUTS, limits
# limits_for), measured by reference_gap_limited below: 3.40e-14 applied, 6.54e-14 demanded.  Over the same cases thrust is
# cut in 2-332 samples of the checked members and the moment in 2-9, the two checkers' cut patterns are identical, and no
# demand comes closer to its bound than 8.2e-6 of the largest demand deviation; the device may be 16x the gap
REF_GAP_LIM = 6.6e-14
PARITY_T, PARITY_B = (3, 17, 33, 200), (1, 64, 65, 130)
EDGE_T, EDGE_B = (4, 16, 18, 32), 65
PARITY_RUNS = [(T, B) for T in PARITY_T for B in PARITY_B] + [(T, EDGE_B) for T in EDGE_T]
# The limits of the Monte Carlo ("limits C"): every member is cut in thrust, 88 % in moment, none leaves the domain
MC_LO, MC_HI, MC_RATE = np.array([40.0, -60.0]), np.array([340.0, 200.0]), np.array([4000.0, 30000.0])
# The moment-only limits of the lane-isolation test: thrust is never cut, so a member is cut where its moment demand is
ISO_LO, ISO_HI, ISO_RATE = np.array([-np.inf, U_MIN[1]]), np.array([np.inf, U_MAX[1]]), INF2


# With 1 or 64 members the checked members are 0 (and 1, 62, 63), whose moment demand never goes below -206 (member 0 at
# sample 0: -205.4 without measurement noise, -189.4 .. -190.3 with it; then -158.8 .. -153.3 at sample 1), so U_MIN[1] = -260
# leaves the moment uncut in all twelve runs of every such size (measured: 0 cut samples).  These sizes take a lower moment
# limit of -100 instead, which cuts member 0 at samples 0 and 1 of every case; everything else is the fixed limits.
U_MIN_SMALL = np.array([U_MIN[0], -100.0])


def limits_for(T, B):
    """lo, hi, rate of a parity case: the fixed limits of tests/test_limits_abi.py, except for B = 1 and 64, where they leave
    the moment uncut among the checked members (U_MIN_SMALL above)"""
    return (U_MIN_SMALL if B in (1, 64) else U_MIN), U_MAX, U_RATE


def lqg_loop_limited(mdl, xo, uo, KK, L, jac, x0, lo, hi, rate, est_input, ehat0=None, dist=None, meas=None, dtype=np.float64,
                     linear=False, bounds=None):
    """The loop of aoc_track_ensemble_lqg_limited for M members about ONE optimum: the arguments of lqg_loop, lo, hi, rate
    (2,) with s = rate * mdl.dt formed once, est_input "applied" or "demanded".  The estimate, L nu, F e and the correction
    are computed in `dtype`, the plant, the demand and the cut in fp64.  linear=True: the plant is x' = xp + A dx + B du.
    bounds: a dict that receives a, b (M,2,T), the bounds each demand was compared with.
    -> xx (M,6,T), uu (M,2,T) the applied input, vv (M,2,T) the demand, xhat (M,6,T), err (M,6,T), cut (M,2,T) bool."""
    assert est_input in EST_INPUTS
    A, B, xp = (a.astype(dtype) for a in jac)
    M, T = x0.shape[0], xo.shape[1]
    K, Lt = np.asarray(KK).astype(dtype), np.asarray(L).astype(dtype)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    s = np.asarray(rate, dtype=np.float64) * np.float64(mdl.dt)
    xx, uu, vv = np.zeros((M, 6, T)), np.zeros((M, 2, T)), np.zeros((M, 2, T))
    cut = np.zeros((M, 2, T), dtype=bool)
    al, bl = np.zeros((M, 2, T)), np.zeros((M, 2, T))
    xhat, err = np.zeros((M, 6, T), dtype), np.zeros((M, 6, T), dtype)
    xx[:, :, 0] = x0
    em = np.zeros((M, 6), dtype) if ehat0 is None else np.broadcast_to(np.asarray(ehat0).astype(dtype), (M, 6)).copy()
    with np.errstate(invalid="ignore"):
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
                v = uo[r, t] + a
                if t == 0:
                    a_, b_ = np.full(M, lo[r]), np.full(M, hi[r])
                else:
                    up = uu[:, r, t - 1]
                    a_ = np.where(up - s[r] > lo[r], up - s[r], lo[r])
                    b_ = np.where(up + s[r] < hi[r], up + s[r], hi[r])
                vv[:, r, t], al[:, r, t], bl[:, r, t] = v, a_, b_
                cut[:, r, t] = (v < a_) | (v > b_)
                uu[:, r, t] = np.where(v < a_, a_, np.where(v > b_, b_, v))
            if linear:
                xn = jac[2][t] + dx @ jac[0][t].T + (uu[:, :, t] - uo[:, t]) @ jac[1][t].T
                xx[:, :, t + 1] = xn if dist is None else xn + dist[:, :, t]
            else:
                for b in range(M):
                    xn = orc.step(mdl, xx[b, :, t], uu[b, :, t])[0]
                    xx[b, :, t + 1] = xn if dist is None else xn + dist[b, :, t]
            F = A[t] + B[t] @ K[:, :, t]
            c = xp[t] - xo[:, t + 1].astype(dtype)
            em = ep @ F.T + c
            if est_input == "applied":
                g = uu[:, :, t].astype(dtype) - vv[:, :, t].astype(dtype)
                told = em.copy()
                told[:, 2] = em[:, 2] + B[t][2, 0] * g[:, 0]
                told[:, 5] = em[:, 5] + B[t][5, 0] * g[:, 0]
                told[:, 4] = em[:, 4] + B[t][4, 1] * g[:, 1]
                em = np.where((cut[:, 0, t] | cut[:, 1, t])[:, None], told, em)
    if bounds is not None:
        bounds.update(a=al, b=bl)
    return xx, uu, vv, xhat, err, cut


def sat_of(vv, uu, cut):
    """(M,2,T) x 3 -> sat (M,6): the number of cut samples, the first (T if none), max_t |v - u| with a NaN that sticks"""
    T = cut.shape[2]
    with np.errstate(invalid="ignore"):
        gap = np.abs(vv - uu)[:, :, :T - 1]
        maxd = np.where(np.isnan(gap).any(axis=2), np.nan, np.fmax.reduce(gap, axis=2))
    first = np.where(cut.any(axis=2), cut.argmax(axis=2), T).astype(np.float64)
    return np.concatenate([cut.sum(axis=2).astype(np.float64), first, maxd], axis=1)


def checker_limited(mdl, XO, UO, KK, L, jac, d, mpo, sel, e0, dist, meas, lims, est_input, dtype=np.float64, bounds=None):
    """lqg_loop_limited on the members `sel`, each about its own optimum -> xx, uu, xhat (len(sel),.,T), est_stats
    (len(sel),12), vv, cut (len(sel),2,T); bounds: a list that receives each member's (a, b)"""
    from test_gpu_lqg import est_stats_of
    out = [[], [], [], [], [], []]
    for b in sel:
        k = b // mpo
        bd = {}
        xx, uu, vv, xh, err, cut = lqg_loop_limited(mdl, XO[k], UO[k], KK[k], L[k], jac[k], (XO[k][:, 0] + d[b])[None], *lims,
                                                    est_input, None if e0 is None else e0[k],
                                                    None if dist is None else dist[b][None],
                                                    None if meas is None else meas[b][None], dtype, bounds=bd)
        for o, v in zip(out, (xx[0], uu[0], xh[0], est_stats_of(err)[0], vv[0], cut[0])):
            o.append(v)
        if bounds is not None:
            bounds.append((bd["a"][0], bd["b"][0]))
    return tuple(np.stack(o) for o in out)


def reference_gap_limited(runs=None, report=None):
    """The checker's own rounding over the GPU parity cases, on the host's restatement of the device's draws, per value of
    est_input -> {est_input: gap}.  On the way it collects, per case, what
    test_the_reference_gap_and_the_conditions_of_the_parity_fixture asserts: report[(T, B, case, est_input)] = (cut samples of thrust, of moment, flips of the cut pattern between the
    fp64 and the long-double checker, the smallest |v - bound| / max |v - u_opt|)."""
    from test_gpu_lqg import CASES, case_inputs, host_draws, scaled_gap, selection, setup
    worst = dict.fromkeys(EST_INPUTS, 0.0)
    for T, B in (PARITY_RUNS if runs is None else runs):
        XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(T, B)
        sel, lims = selection(B), limits_for(T, B)
        for name in CASES:
            sigma, rho, e0 = case_inputs(name, T, B, n_opt)
            dist, meas = host_draws(B, T, sigma, rho)
            for est_input in EST_INPUTS:
                bd = []
                a = checker_limited(mdl, XO, UO, KK, L, jac, d, mpo, sel, e0, dist, meas, lims, est_input, bounds=bd)
                b = checker_limited(mdl, XO, UO, KK, L, jac, d, mpo, sel, e0, dist, meas, lims, est_input, np.longdouble)
                margin = np.inf
                for i, m in enumerate(sel):
                    k = m // mpo
                    worst[est_input] = max(worst[est_input], scaled_gap([v[i:i + 1] for v in a[:4]], [v[i:i + 1] for v in b[:4]],
                                                                        XO[k], UO[k]))
                    v, (lo_t, hi_t) = a[4][i][:, :T - 1], [x[:, :T - 1] for x in bd[i]]
                    scale = np.abs(v - UO[k][:, :T - 1]).max(axis=1, keepdims=True)
                    margin = min(margin, float((np.minimum(np.abs(v - lo_t), np.abs(v - hi_t)) / scale).min()))
                if report is not None:
                    report[(T, B, name, est_input)] = (int(a[5][:, 0].sum()), int(a[5][:, 1].sum()), int((a[5] != b[5]).sum()), margin)
    return worst


def _prob(T=10, B=64):
    p = _lib.Problem()
    p.B, p.T = B, T
    p.model.dt = 1e-3
    return p


def _limits(lo=(-1.0, -1.0), hi=(1.0, 1.0), rate=(1.0, 1.0)):
    return _lib.ActuatorLimits((C.c_double * 2)(*lo), (C.c_double * 2)(*hi), (C.c_double * 2)(*rate))


def test_abi_revision_symbols_and_the_scratch_query():
    _lib.build_library()
    lib = _lib.lib()
    assert lib.aoc_abi_version() == _lib.AOC_ABI_VERSION == 5
    assert (_lib.EST_INPUT_DEMANDED, _lib.EST_INPUT_APPLIED) == (0, 1)
    for name in ("aoc_track_ensemble_lqg_limited", "aoc_track_ensemble_lqg_limited_scratch_bytes"):
        assert name in _lib.SYMBOLS and callable(getattr(lib, name))
    assert len(_lib.SYMBOLS["aoc_track_ensemble_lqg_limited"][1]) == 23
    # the two calls it joins keep their argument lists
    assert len(_lib.SYMBOLS["aoc_track_ensemble_lqg"][1]) == 19 and len(_lib.SYMBOLS["aoc_track_ensemble_limited"][1]) == 20
    hdr = open(_lib._HDR).read()
    assert "#define AOC_ABI_VERSION 5" in hdr and "enum { AOC_EST_INPUT_DEMANDED = 0, AOC_EST_INPUT_APPLIED = 1 };" in hdr
    assert "still 5, an addition: aoc_track_ensemble_lqg_limited" in hdr
    assert "Not covered: limits in the loop of aoc_track_ensemble_lqg" not in hdr
    q = lib.aoc_track_ensemble_lqg_limited_scratch_bytes
    nt, T = 6, 33                                                    # B = 322 members about two optima
    assert q(322, 2, T, 192, 0) == lib.aoc_track_ensemble_lqg_scratch_bytes(2, T) == 2 * T * REC
    assert q(322, 2, T, 192, 1) == 2 * T * REC + nt * T * 8
    assert q(64, 1, 3, 64, 1) == 3 * REC + 3 * 8 and q(1, 1, 3, 64, 1) == 3 * REC + 3 * 8
    assert q(130, 3, 17, 64, 1) == 3 * 17 * REC + 3 * 17 * 8
    assert (3 * 17 * REC) % 16 == 0                                  # a record is 448 bytes: the rounding never adds
    assert q(1 << 24, 1 << 18, 1 << 12, 64, 1) == (1 << 30) * REC + (1 << 18) * (1 << 12) * 8   # no 32-bit product on the way
    for bad in ((0, 1, T, 64, 1), (64, 0, T, 64, 1), (64, 1, 2, 64, 1), (64, 1, T, 100, 1), (64, 1, T, 32, 1), (65, 1, T, 64, 1),
                (64, 2, T, 64, 1)):
        assert q(*bad) == 0, bad


def test_refusals_carry_a_reason_in_their_order():
    """first the refusals of aoc_track_ensemble_lqg in its order (scratch against this call's own size), then those of the
    limits in the texts of aoc_track_ensemble_limited, then est_input"""
    lib = _lib.lib()
    big = 1 << 40
    nan, inf = float("nan"), float("inf")
    six = lambda *v: (C.c_double * 6)(*v)
    nz = _lib.MpcNoise(1, 0, 0, six(0, 0, 0, 0, 0, 0))

    def call(p, n_opt=1, mpo=64, nominal=16, filter=16, x0_reg=16, ehat0=None, noise=None, rho=None, limits=_limits(),
             est_input=1, x_reg=None, u_reg=None, xhat=None, dist=None, meas=None, stats=16, est_stats=16, sat=16,
             sat_count=None, status=None, scratch=16, scratch_bytes=big):
        return lib.aoc_track_ensemble_lqg_limited(C.byref(p) if p is not None else None, n_opt, mpo, nominal, filter, x0_reg,
                                                  ehat0, C.byref(noise) if noise is not None else None, rho,
                                                  C.byref(limits) if limits is not None else None, est_input, x_reg, u_reg,
                                                  xhat, dist, meas, stats, est_stats, sat, sat_count, status, scratch,
                                                  scratch_bytes)
    need = lib.aoc_track_ensemble_lqg_limited_scratch_bytes(128, 2, 10, 64, 1)
    assert need == 2 * 10 * REC + 2 * 10 * 8
    f32 = _prob()
    f32.x_out_f32 = 1
    skew = _prob()
    skew.RRt[1], skew.RRt[2] = 1.0, 2.0
    cases = [
        # the refusals of aoc_track_ensemble_lqg, each before every new one (limits = NULL rides along)
        (dict(p=None, limits=None), b"aoc_problem is NULL"),
        (dict(p=_prob(), nominal=None, limits=None), b"nominal is NULL"),
        (dict(p=_prob(), x0_reg=None, sat=None), b"x0_reg is NULL"),
        (dict(p=_prob(), stats=None, limits=None), b"stats is NULL"),
        (dict(p=_prob(), filter=None, limits=None), b"filter is NULL"),
        (dict(p=_prob(), est_stats=None, sat=None), b"est_stats is NULL"),
        (dict(p=_prob(), n_opt=0, limits=None), b"n_opt = 0"),
        (dict(p=_prob(), mpo=96, limits=None), b"members_per_opt = 96"),
        (dict(p=_prob(T=2), limits=None), b"T = 2"),
        (dict(p=_prob(B=65), limits=None), b"B = 65 members do not fill"),
        (dict(p=_prob(), x_reg=16, limits=None), b"x_reg and u_reg go together"),
        (dict(p=f32, x_reg=16, u_reg=16, noise=nz, limits=None), b"float32 state storage"),
        (dict(p=skew, limits=None), b"RRt is not symmetric"),
        (dict(p=_prob(), rho=six(1, 1, 1, 1, 1, 1), limits=None), b"rho without noise"),
        (dict(p=_prob(), noise=nz, rho=six(1, 1, -1.0, 1, 1, 1), est_input=7), b"rho[2]"),
        (dict(p=_prob(), scratch=None, limits=None),
         b"scratch is NULL (need %d bytes, aoc_track_ensemble_lqg_limited_scratch_bytes)" % (10 * REC)),
        (dict(p=_prob(), scratch=None, sat_count=16), b"scratch is NULL (need %d bytes" % (10 * REC + 80)),
        (dict(p=_prob(), scratch=24, limits=None), b"16-byte aligned"),
        (dict(p=_prob(B=128), n_opt=2, sat_count=16, scratch_bytes=need - 1, limits=None),
         b"scratch_bytes = %d, need %d (aoc_track_ensemble_lqg_limited_scratch_bytes)" % (need - 1, need)),
        (dict(p=_prob(B=128), n_opt=2, scratch_bytes=need - 161, limits=None), b"scratch_bytes = %d, need %d" % (need - 161, need - 160)),
        # the new ones, in their order
        (dict(p=_prob(), limits=None, sat=None, est_input=7), b"limits is NULL"),
        (dict(p=_prob(), sat=None, limits=_limits(lo=(nan, 0.0)), est_input=7), b"sat is NULL"),
        (dict(p=_prob(), limits=_limits(lo=(nan, 2.0)), est_input=7), b"NaN in channel 0"),
        (dict(p=_prob(), limits=_limits(hi=(1.0, nan), rate=(1.0, 0.0))), b"NaN in channel 1"),
        (dict(p=_prob(), limits=_limits(rate=(nan, 1.0))), b"NaN in channel 0"),
        (dict(p=_prob(), limits=_limits(lo=(2.0, -1.0), rate=(0.0, 1.0))), b"limits.lo[0] = 2 > limits.hi[0] = 1"),
        (dict(p=_prob(), limits=_limits(lo=(-1.0, inf))), b"limits.lo[1] = inf > limits.hi[1] = 1"),
        (dict(p=_prob(), limits=_limits(rate=(0.0, 1.0)), est_input=7), b"limits.rate[0] = 0"),
        (dict(p=_prob(), limits=_limits(rate=(1.0, -inf))), b"limits.rate[1] = -inf"),
        (dict(p=_prob(), est_input=2), b"est_input = 2"),
        (dict(p=_prob(), est_input=-1), b"est_input = -1"),
    ]
    for kw, reason in cases:
        # leave another reason behind first, so that an error return without a new reason shows
        q = _lib.Problem()
        q.B, q.T, q.ref = 4, 2, 1
        assert lib.aoc_traj_cost(C.byref(q), 1, 1, 1, 1) == -1 and b"T = 2 " in lib.aoc_last_hip_error() + b" "
        assert call(**kw) == -1, kw
        msg = lib.aoc_last_hip_error()
        assert msg.startswith(b"aoc_track_ensemble_lqg_limited: ") and reason in msg, (kw, msg)
    # the two calls it joins still name themselves
    assert lib.aoc_track_ensemble_lqg(C.byref(_prob()), 1, 64, 16, None, 16, None, None, None, None, None, None, None, None, 16,
                                      16, None, 16, big) == -1
    assert lib.aoc_last_hip_error().startswith(b"aoc_track_ensemble_lqg: filter is NULL")


def test_keyword_rules():
    """the keyword checks of batch.track_ensemble come before anything touches a device"""
    from aircraftoptimalcontrol_amd import batch

    class P:
        device, T = "cpu", 5
    xo, uo, L, d = np.zeros((6, 5)), np.zeros((2, 5)), np.zeros((6, 6, 5)), np.zeros((4, 6))
    lim = dict(u_max=(1.0, None))
    with pytest.raises(ValueError, match=r"filter=.*u_min= / u_max= / u_rate=.*est_input="):
        batch.track_ensemble(P(), xo, uo, delta=d, filter=L, **lim)
    for kw in (dict(est_input="applied"), dict(est_input="applied", filter=L), dict(est_input="demanded", **lim)):
        with pytest.raises(ValueError, match=r"est_input= goes with filter= and a limit"):
            batch.track_ensemble(P(), xo, uo, delta=d, **kw)
    for name in ("Applied", "", 1, "told"):
        with pytest.raises(ValueError, match=r'est_input=.*"applied" and "demanded"'):
            batch.track_ensemble(P(), xo, uo, delta=d, filter=L, est_input=name, **lim)
    for kw in (dict(envelope=True), dict(quantiles=(0.5,)), dict(predict=True)):
        with pytest.raises(ValueError, match="does not combine with envelope=, quantiles= or predict="):
            batch.track_ensemble(P(), xo, uo, delta=d, filter=L, est_input="applied", **lim, **kw)
    with pytest.raises(ValueError):                                  # malformed limits are still refused
        batch.track_ensemble(P(), xo, uo, delta=d, filter=L, est_input="applied", u_min=(1.0, 0.0), u_max=(0.0, 0.0))
    assert "est_input" in batch.track_ensemble.__doc__ and "WITHOUT limits" in batch.track_ensemble.__doc__


@pytest.fixture(scope="module")
def g4_64():
    """g4's first 200 samples, deltas(64), SIGMA, RHO and the host's restatement of the device's draws, computed once"""
    from test_gpu_ensemble import SIGMA
    from test_gpu_lqg import RHO, host_draws, setup
    XO, UO, KK, L, jac, d, n_opt, mpo, mdl = setup(200, 64)
    dist, meas = host_draws(64, 200, SIGMA, RHO)
    return mdl, XO[0], UO[0], KK[0], L[0], jac[0], XO[0][:, 0] + d, dist, meas


def test_checker_with_infinite_limits_is_lqg_loop(g4_64):
    """both values of est_input, twelve members, with an ehat0: every array of lqg_loop bit for bit, no sample cut"""
    from test_gpu_ensemble import DELTA_SCALE
    from test_gpu_lqg import lqg_loop
    mdl, xo, uo, KK, L, jac, x0, dist, meas = g4_64
    m, e0 = slice(0, 12), 0.5 * DELTA_SCALE
    want = lqg_loop(mdl, xo, uo, KK, L, jac, x0[m], e0, dist[m], meas[m])
    for est_input in EST_INPUTS:
        xx, uu, vv, xhat, err, cut = lqg_loop_limited(mdl, xo, uo, KK, L, jac, x0[m], -INF2, INF2, INF2, est_input, e0, dist[m],
                                                      meas[m])
        for got, w in zip((xx, uu, xhat, err), want):
            assert np.array_equal(got, w), est_input
        assert np.array_equal(vv, uu) and not cut.any()


def test_on_a_linear_plant_the_informed_estimator_does_not_see_the_limits(g4_64):
    """The plant x' = xp + A dx + B du, everything else the same: the error sequence of the estimator that is told the
    applied input equals that of the loop without limits to 1e-13 of each channel's scale (max |dx_c| of that loop — the
    scale of scaled_gap), although thrust and moment are cut; the one left with its demand differs by more than 1e-3 in
    channel 4."""
    mdl, xo, uo, KK, L, jac, x0, dist, meas = g4_64
    run = lambda lo, hi, rate, est: lqg_loop_limited(mdl, xo, uo, KK, L, jac, x0, lo, hi, rate, est, None, dist, meas, linear=True)
    free = run(-INF2, INF2, INF2, "applied")
    told, left = run(U_MIN, U_MAX, U_RATE, "applied"), run(U_MIN, U_MAX, U_RATE, "demanded")
    assert told[5][:, 0].any() and told[5][:, 1].any() and not free[5].any()
    assert np.abs(told[0] - free[0]).max() > 1e-3                       # the trajectories do differ
    scale = np.abs(free[0] - xo[None]).max(axis=(0, 2))
    gap_told = np.abs(told[4] - free[4]).max(axis=(0, 2)) / scale
    gap_left = np.abs(left[4] - free[4]).max(axis=(0, 2))
    print("linear plant: informed %.3g of the channel scale, uninformed %s absolute" % (gap_told.max(), np.round(gap_left, 4)))
    assert gap_told.max() <= 1e-13, gap_told
    assert gap_left[4] > 1e-3, gap_left


def test_the_reference_gap_and_the_conditions_of_the_parity_fixture():
    """REF_GAP_LIM is the checker's own rounding over the GPU parity cases: nothing measured exceeds the constant and the
    constant is not padded beyond 2x what is measured.  And the conditions that let the GPU tests compare sat[0..3] and
    sat_count EXACTLY and leave no member out: in every case both channels are cut at least once among the checked members,
    the fp64 and the long-double checker give the identical cut pattern, and no demand comes closer to the bound it is
    compared with than 1e-7 of the largest demand deviation."""
    report = {}
    gap = reference_gap_limited(report=report)
    print("checker fp64 against long double: applied %.3g, demanded %.3g (REF_GAP_LIM %.3g)" % (gap["applied"], gap["demanded"], REF_GAP_LIM))
    n0, n1, flips, margin = (np.array([v[i] for v in report.values()]) for i in range(4))
    print("cut samples: thrust %d-%d, moment %d-%d; flips %d; smallest margin %.3g" % (n0.min(), n0.max(), n1.min(), n1.max(),
                                                                                     flips.sum(), margin.min()))
    for key, (c0, c1, fl, mg) in report.items():
        assert c0 >= 1 and c1 >= 1, (key, c0, c1)
        assert fl == 0, (key, fl)
        assert mg >= 1e-7, (key, mg)
    worst = max(gap.values())
    assert 0.5 * REF_GAP_LIM <= worst <= REF_GAP_LIM, gap


def test_the_moment_only_limits_cut_some_members_and_spare_others(g4_64):
    """What the lane-isolation test of tests/test_gpu_lqg_limits.py relies on: among 64 members at T = 200 under ISO_LO /
    ISO_HI at least 8 are cut and at least 8 are never cut, for both values of est_input"""
    mdl, xo, uo, KK, L, jac, x0, dist, meas = g4_64
    for est_input in EST_INPUTS:
        cut = lqg_loop_limited(mdl, xo, uo, KK, L, jac, x0, ISO_LO, ISO_HI, ISO_RATE, est_input, None, dist, meas)[5]
        n = int(cut.any(axis=(1, 2)).sum())
        print("%s: %d of 64 members cut" % (est_input, n))
        assert not cut[:, 0].any() and 8 <= n <= 56, (est_input, n)


@pytest.fixture(scope="module")
def mc_inputs():
    from aircraftoptimalcontrol_amd import mpc
    from test_gpu_covariance import MC_M, MC_SEED, MC_T, g4_jacobians, mc_members
    from test_gpu_ensemble import SIGMA
    from test_gpu_lqg import RHO, mc_gains
    g, mdl, (A, B, xp) = g4_jacobians()
    T, M = MC_T, MC_M
    xo, uo, KK, L, P_post = mc_gains(0.1)
    dist = np.zeros((M, 6, T))
    for t in range(T - 1):
        dist[:, :, t] = mpc.noise_draws(MC_SEED, t, 0, M, SIGMA)
    meas = np.stack([mpc.noise_draws(MC_SEED, t, 0, M, RHO, 1) for t in range(T)], axis=2)
    return mdl, xo, uo, KK, L, (A[:T - 1], B[:T - 1], xp[:T - 1]), xo[:, 0] + mc_members(0.1)[0], dist, meas, P_post


@pytest.mark.parametrize("est_input", EST_INPUTS)
def test_host_checker_under_limits_against_the_filters_own_covariance(mc_inputs, est_input):
    """The Monte Carlo of tests/test_lqg_abi.py (2048 members, T = 200, s = 0.1, mc_gains(0.1), MC_SEED) under the limits
    MC_LO / MC_HI / MC_RATE, which cut every member in thrust and most in moment and let none leave the domain: the error of
    the estimator that is told the applied input agrees with the filter's own P^+ and 0 within sampling error (z_cov, z_mean
    <= 5 — what the loop WITHOUT limits gives), the one left with its demand does not (z_cov >= 15)."""
    from test_gpu_lqg import mc_z
    mdl, xo, uo, KK, L, jac, x0, dist, meas, P_post = mc_inputs
    xx, uu, vv, xhat, err, cut = lqg_loop_limited(mdl, xo, uo, KK, L, jac, x0, MC_LO, MC_HI, MC_RATE, est_input, None, dist, meas)
    zc, zm = mc_z(err, P_post)
    frac = cut.any(axis=2).mean(axis=0)
    print("%s: z_cov = %.3g, z_mean = %.3g, members cut %s" % (est_input, zc, zm, frac))
    assert frac[0] > 0.9 and frac[1] > 0.5 and (xx[:, 2] > 0).all() and np.isfinite(xx).all()
    if est_input == "applied":
        assert zc <= 5 and zm <= 5, (zc, zm)
    else:
        assert zc >= 15, zc
