"""CPU-side checks of aoc_track_ensemble_limited (actuator limits and rate limits in the tracking ensembles' loop): the
symbol binds and the struct has its size, every new refusal arrives with its reason before anything touches a device,
batch.track_ensemble refuses filter= together with a limit, the merge and summary helpers do what they say, and the
checker of tests/test_gpu_limits.py — host_loop_limited below — is host_loop where nothing is cut and meets the conditions
the GPU fixtures rely on.

The fixed limits.  U_MIN / U_MAX are the magnitude limits the feature was specified with.  U_RATE is frozen from a
measurement: the 0.9 quantile over the members of max_t |v_t - v_{t-1}| / dt of the UNLIMITED host loop (g4's first 200
samples, deltas(192), no noise) is 8179.6 in thrust and 68954.6 in pitching moment (medians 4318.9 / 28037.4, maxima
11235.0 / 106889.3); rounded to two significant digits that is (8200, 69000) input units per second, 8.2 and 69 per sample at
dt = 1e-3.  test_the_rate_constant_is_the_measured_quantile restates the measurement."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as orc
from aircraftoptimalcontrol_amd import _lib

U_MIN = np.array([-140.0, -260.0])
U_MAX = np.array([360.0, 430.0])
U_RATE = np.array([8200.0, 69000.0])
INF2 = np.full(2, np.inf)


def host_loop_limited(mdl, xo, uo, KK, x0, lo, hi, rate, dist=None):
    """host_loop of tests/test_gpu_ensemble.py with the selection of include/aoc.h between forming the demand and stepping:
    lo, hi, rate (2,), s = rate * mdl.dt formed once.  -> xx (M,6,T), uu (M,2,T) (the applied input; sample T-1 zero),
    vv (M,2,T) (the demand; sample T-1 zero), and the three cut statistics ncut (M,2), first (M,2) (T if none), maxd (M,2) =
    max_t |v - u| with a NaN that sticks, and cut (M,2,T) bool."""
    M, T = x0.shape[0], xo.shape[1]
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    s = np.asarray(rate, dtype=np.float64) * np.float64(mdl.dt)
    xx, uu, vv = np.zeros((M, 6, T)), np.zeros((M, 2, T)), np.zeros((M, 2, T))
    cut = np.zeros((M, 2, T), dtype=bool)
    xx[:, :, 0] = x0
    with np.errstate(invalid="ignore"):
        for t in range(T - 1):
            d = xx[:, :, t] - xo[:, t]
            for r in range(2):
                a = np.zeros(M)
                for c in range(6):
                    a = a + KK[r, c, t] * d[:, c]
                v = uo[r, t] + a
                if t == 0:
                    al, bl = np.full(M, lo[r]), np.full(M, hi[r])
                else:
                    up = uu[:, r, t - 1]
                    al = np.where(up - s[r] > lo[r], up - s[r], lo[r])
                    bl = np.where(up + s[r] < hi[r], up + s[r], hi[r])
                vv[:, r, t] = v
                cut[:, r, t] = (v < al) | (v > bl)
                uu[:, r, t] = np.where(v < al, al, np.where(v > bl, bl, v))
            for b in range(M):
                xn = orc.step(mdl, xx[b, :, t], uu[b, :, t])[0]
                xx[b, :, t + 1] = xn if dist is None else xn + dist[b, :, t]
        ncut = cut.sum(axis=2).astype(np.float64)
        first = np.where(cut.any(axis=2), cut.argmax(axis=2), T).astype(np.float64)
        gap = np.abs(vv - uu)[:, :, :T - 1]
        maxd = np.where(np.isnan(gap).any(axis=2), np.nan, np.fmax.reduce(gap, axis=2))
    return xx, uu, vv, ncut, first, maxd, cut


def _g4_200():
    g = load_golden("g4_lqr_tracking")
    T = 200
    return g, orc.default_model(float(g["dt"])), g["xx_opt"][:, :T], g["uu_opt"][:, :T], g["KK"][:, :, :T]


@pytest.fixture(scope="module")
def loops():
    """The checker on g4's first 200 samples with deltas(192): unlimited (host_loop), magnitude, rate, both — computed once"""
    from test_gpu_ensemble import deltas, host_loop
    g, mdl, xo, uo, KK = _g4_200()
    x0 = xo[:, 0] + deltas(192)
    run = lambda lo, hi, rate: host_loop_limited(mdl, xo, uo, KK, x0, lo, hi, rate)
    return dict(plain=host_loop(mdl, xo, uo, KK, x0), none=run(-INF2, INF2, INF2), mag=run(U_MIN, U_MAX, INF2),
                rate=run(-INF2, INF2, U_RATE), both=run(U_MIN, U_MAX, U_RATE), dt=float(g["dt"]))


def _prob(B=64, T=10):
    p = _lib.Problem()
    p.B, p.T = B, T
    p.model.dt = 1e-3
    p.RRt[:] = [1e-5, 0.0, 0.0, 1e-5]
    return p


def _limits(lo=(-1.0, -1.0), hi=(1.0, 1.0), rate=(1.0, 1.0)):
    return _lib.ActuatorLimits((C.c_double * 2)(*lo), (C.c_double * 2)(*hi), (C.c_double * 2)(*rate))


def test_symbol_binds_and_the_struct_is_48_bytes():
    _lib.build_library()
    lib = _lib.lib()
    assert lib.aoc_abi_version() == _lib.AOC_ABI_VERSION == 5
    assert C.sizeof(_lib.ActuatorLimits) == 48 and _lib.AOC_SAT_NSTAT == 6
    assert "aoc_track_ensemble_limited" in _lib.SYMBOLS and "aoc_ensemble_limited_scratch_bytes" in _lib.SYMBOLS
    assert callable(lib.aoc_track_ensemble_limited)
    q = lib.aoc_ensemble_limited_scratch_bytes
    nt, T = 6, 33                                                    # B = 322 members
    assert q(0, 322, T, 192, 0) == 0 and q(0, 322, T, 192, 1) == nt * T * 8
    assert q(1, 322, T, 192, 0) == lib.aoc_ensemble_envelope_scratch_bytes(322, T, 192) == nt * T * 352
    assert q(1, 322, T, 192, 1) == nt * T * (352 + 8)
    assert q(2, 322, T, 192, 1) == lib.aoc_ensemble_histogram_scratch_bytes(322, T, 192) + nt * T * 8
    assert q(3, 322, T, 192, 1) == 0 and q(0, 322, T, 100, 1) == 0 and q(0, 0, T, 64, 1) == 0


def test_new_refusals_carry_a_reason_and_the_old_ones_still_come_first():
    _lib.build_library()
    lib = _lib.lib()
    nan, inf = float("nan"), float("inf")

    def call(p, mode=0, n_opt=1, mpo=64, nominal=1, x0=1, noise=None, limits=_limits(), bins=None, x=None, u=None,
             dist=None, stats=1, status=None, sat=1, sat_count=None, envelope=None, hist=None, scratch=None, nbytes=0):
        return lib.aoc_track_ensemble_limited(C.byref(p) if p is not None else None, mode, n_opt, mpo, nominal, x0, noise,
                                              C.byref(limits) if limits is not None else None, bins, x, u, dist, stats,
                                              status, sat, sat_count, envelope, hist, scratch, nbytes)
    rsym = _prob()
    rsym.RRt[1] = 1e-7
    cases = [
        # the new ones
        (dict(p=_prob(), limits=None), b"limits is NULL"),
        (dict(p=_prob(), sat=None), b"sat is NULL"),
        (dict(p=_prob(), limits=_limits(lo=(nan, -1.0))), b"NaN in channel 0"),
        (dict(p=_prob(), limits=_limits(hi=(1.0, nan))), b"NaN in channel 1"),
        (dict(p=_prob(), limits=_limits(rate=(nan, 1.0))), b"NaN in channel 0"),
        (dict(p=_prob(), limits=_limits(lo=(2.0, -1.0))), b"limits.lo[0] = 2 > limits.hi[0] = 1"),
        (dict(p=_prob(), limits=_limits(lo=(-1.0, inf))), b"limits.lo[1] = inf > limits.hi[1] = 1"),
        (dict(p=_prob(), limits=_limits(rate=(0.0, 1.0))), b"limits.rate[0] = 0"),
        (dict(p=_prob(), limits=_limits(rate=(1.0, -3.0))), b"limits.rate[1] = -3"),
        (dict(p=_prob(), limits=_limits(rate=(1.0, -inf))), b"limits.rate[1] = -inf"),
        (dict(p=_prob(), mode=3), b"mode = 3"),
        (dict(p=_prob(), sat_count=1), b"scratch is NULL (need 80 bytes, aoc_ensemble_limited_scratch_bytes)"),
        (dict(p=_prob(), sat_count=1, scratch=16, nbytes=79), b"scratch_bytes = 79, need 80"),
        # those of the calls it carries, in their order: a NULL problem before NULL limits, NULL limits before the geometry
        (dict(p=None, limits=None), b"aoc_problem is NULL"),
        (dict(p=_prob(), nominal=None, limits=None), b"nominal is NULL"),
        (dict(p=_prob(), x0=None), b"x0_reg is NULL"),
        (dict(p=_prob(), stats=None, sat=None), b"stats is NULL"),
        (dict(p=_prob(T=2), limits=None), b"limits is NULL"),
        (dict(p=_prob(), n_opt=0), b"n_opt = 0"),
        (dict(p=_prob(), mpo=100), b"members_per_opt = 100"),
        (dict(p=_prob(T=2)), b"T = 2"),
        (dict(p=_prob(B=65)), b"B = 65"),
        (dict(p=_prob(), x=1), b"x_reg and u_reg go together"),
        (dict(p=rsym), b"RRt is not symmetric"),
        (dict(p=_prob(T=2), limits=_limits(rate=(0.0, 1.0))), b"T = 2"),
        (dict(p=_prob(), mode=1), b"envelope is NULL"),
        (dict(p=_prob(), mode=1, envelope=1), b"scratch is NULL (need 3520 bytes, aoc_ensemble_limited_scratch_bytes)"),
        (dict(p=_prob(), mode=2), b"bins is NULL"),
        (dict(p=_prob(), mode=2, bins=1), b"hist is NULL"),
        (dict(p=_prob(), mode=2, bins=1, hist=16, scratch=8, nbytes=1 << 20), b"16-byte aligned"),
    ]
    for kw, reason in cases:
        # leave another reason behind first, so that an error return without a new reason shows
        q = _lib.Problem()
        q.B, q.T, q.ref = 4, 2, 1
        assert lib.aoc_traj_cost(C.byref(q), 1, 1, 1, 1) == -1 and b"T = 2 " in lib.aoc_last_hip_error() + b" "
        assert call(**kw) == -1, kw
        msg = lib.aoc_last_hip_error()
        assert b"aoc_track_ensemble_limited" in msg and reason in msg, (kw, msg)


def test_filter_with_a_limit_and_malformed_limits_are_value_errors():
    from aircraftoptimalcontrol_amd import batch
    L = np.zeros((6, 6, 10))
    for kw in (dict(u_min=(-1.0, -1.0)), dict(u_max=(1.0, None)), dict(u_rate=(np.inf, 5.0))):
        with pytest.raises(ValueError, match=r"filter=.*u_min= / u_max= / u_rate="):
            batch.track_ensemble(None, np.zeros((6, 10)), np.zeros((2, 10)), delta=np.zeros((64, 6)), filter=L, **kw)
    lo, hi, rate = batch.actuator_limits(u_min=(-3.0, None), u_rate=(None, 7.0))
    assert np.array_equal(lo, [-3.0, -np.inf]) and np.array_equal(hi, [np.inf, np.inf]) and np.array_equal(rate, [np.inf, 7.0])
    for kw in (dict(u_min=(1.0,)), dict(u_min=(np.nan, 0.0)), dict(u_min=(1.0, 0.0), u_max=(0.0, 0.0)),
               dict(u_rate=(0.0, 1.0)), dict(u_rate=(1.0, -1.0)), dict(u_max=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            batch.actuator_limits(**kw)


def test_sat_count_merge_and_frac_cut_on_hand_made_arrays():
    from aircraftoptimalcontrol_amd import batch
    a = np.array([[[1, 0], [2, 5], [0, 0]]], dtype=np.int32)
    b = np.array([[[0, 7], [3, 0], [0, 0]]], dtype=np.int32)
    m = batch.sat_count_merge(a, b)
    assert np.array_equal(m, [[[1, 7], [5, 5], [0, 0]]]) and m.dtype == np.int64
    big = np.full((4, 2), 2 ** 31 - 1, dtype=np.int32)
    assert (batch.sat_count_merge(big, big) == 2 ** 32 - 2).all()            # no wrap
    for bad in ((a, b[:, :2]), (a.astype(float), b), (a[..., :1], b[..., :1]), (a[0, 0], b[0, 0][:1])):
        with pytest.raises(ValueError):
            batch.sat_count_merge(*bad)
    sat = np.zeros((5, 6))
    sat[:, 2:4] = 33
    sat[0, 0], sat[3, 0], sat[3, 1] = 4, 1, 9
    assert np.array_equal(batch.frac_cut(sat), [0.4, 0.2])
    assert np.array_equal(batch.frac_cut(np.zeros((3, 6))), [0.0, 0.0])
    with pytest.raises(ValueError):
        batch.frac_cut(np.zeros((3, 5)))


def test_checker_with_infinite_limits_is_host_loop(loops):
    xx, uu = loops["plain"]
    lx, lu, lv, ncut, first, maxd, cut = loops["none"]
    assert np.array_equal(lx, xx) and np.array_equal(lu, uu) and np.array_equal(lv, uu)
    assert not cut.any() and not ncut.any() and (first == 200).all()
    assert not maxd.any() and not np.signbit(maxd).any()


def test_the_rate_constant_is_the_measured_quantile(loops):
    _, uu = loops["plain"]
    slew = np.abs(np.diff(uu[:, :, :199], axis=2)).max(axis=2) / loops["dt"]
    q90 = np.quantile(slew, 0.9, axis=0)
    two_digits = np.array([float("%.1e" % v) for v in q90])
    assert np.array_equal(two_digits, U_RATE), q90


def test_the_demand_of_the_unlimited_loop_is_what_the_issue_measured(loops):
    _, uu = loops["plain"]
    v = uu[:, :, :199]
    assert -679 < v[:, 0].min() < -678 and 976 < v[:, 0].max() < 977
    assert -468 < v[:, 1].min() < -467 and 876 < v[:, 1].max() < 877


@pytest.mark.parametrize("which", ["mag", "rate"])
def test_each_limit_cuts_some_members_and_spares_others(loops, which):
    """What the GPU fixtures rely on: >= 16 members are cut in each channel and >= 16 are never cut (in that channel)"""
    ncut = loops[which][3]
    for r in range(2):
        assert (ncut[:, r] > 0).sum() >= 16, (which, r, (ncut[:, r] > 0).sum())
        assert (ncut[:, r] == 0).sum() >= 16, (which, r, (ncut[:, r] == 0).sum())


def test_with_both_limits_three_quarters_stay_in_the_domain(loops):
    xx = loops["both"][0]
    bad = (~(xx[:, 2, :] > 0) | ~np.isfinite(xx).all(axis=1)).any(axis=1)
    assert (~bad).sum() >= 0.75 * 192, bad.sum()
    lo, hi = U_MIN[None, :, None], U_MAX[None, :, None]
    uu = loops["both"][1][:, :, :199]
    assert ((uu >= lo) & (uu <= hi)).all()
