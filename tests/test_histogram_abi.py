"""CPU-side checks of aoc_track_ensemble_histogram: the ABI revision stays 5 and the symbols are bound, the scratch query
follows its formula, every argument error is reported with its reason before anything touches a device (the new arguments,
and every case of tests/test_ensemble_abi.py through the new entry point), and batch.histogram_bins / histogram_merge /
histogram_quantiles do on NumPy arrays what they say.

numpy_histogram below restates the binning rule of include/aoc.h; tests/test_gpu_histogram.py compares the device's counts
with it on trajectories of aoc_track_ensemble.

Bound of the quantile test, derived, not measured.  The rule v -> k is monotone in v (a subtraction, a multiplication by
inv_w >= 0, a truncation, each monotone), so with r = max(1, ceil(q n)) the r-th order statistic of the members that count
lies in the first bin whose cumulative count reaches r.  Where the bins span min .. max of the values (histogram_bins) that
bin is an interval of one width, and its midpoint is within half a width of every value in it; a whole width of margin
covers the rounding at the edges."""
import ctypes as C

import numpy as np
import pytest

from aircraftoptimalcontrol_amd import _lib

NCH, NBIN = 8, 64


def numpy_histogram(xx, uu, xo, uo, first_bad, group, bins):
    """The counts of include/aoc.h with NumPy: trajectories xx (M,6,T), uu (M,2,T) about the nominals xo (n_opt,6,T) or
    (6,T), uo likewise; member b belongs to optimum group[b] and counts at sample t iff t < first_bad[b]; bins
    (n_opt,T,8,2) = (lo, inv_w).  s = (v - lo) * inv_w in two fp64 operations, k = 63 if s >= 63, int(s) if s >= 1, else 0
    (a NaN fails both comparisons).  -> hist (n_opt,T,8,64) int64; channels 6, 7 at sample T-1 are zero."""
    xx, uu = np.asarray(xx, dtype=np.float64), np.asarray(uu, dtype=np.float64)
    xo, uo = np.asarray(xo, dtype=np.float64), np.asarray(uo, dtype=np.float64)
    if xo.ndim == 2:
        xo, uo = xo[None], uo[None]
    bins = np.asarray(bins, dtype=np.float64)
    first_bad, group = np.asarray(first_bad), np.asarray(group)
    n_opt, T = xo.shape[0], xx.shape[2]
    assert bins.shape == (n_opt, T, NCH, 2)
    hist = np.zeros((n_opt, T, NCH, NBIN), dtype=np.int64)
    tt = np.arange(T)
    for g in range(n_opt):
        m = np.flatnonzero(group == g)
        counts = tt[None, :] < first_bad[m][:, None]                                # (m,T)
        v = np.concatenate([np.subtract(xx[m], xo[g]), np.subtract(uu[m], uo[g])], axis=1)   # (m,8,T)
        lo, inv_w = bins[g, :, :, 0].T, bins[g, :, :, 1].T                          # (8,T)
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.subtract(v, lo[None]) * inv_w[None]
            ge63, ge1 = s >= 63.0, s >= 1.0
            k = np.where(ge63, 63, np.where(ge1, np.where(ge1 & ~ge63, s, 1.0).astype(np.int64), 0))
        for c in range(NCH):
            w = counts if c < 6 else counts & (tt[None, :] < T - 1)
            np.add.at(hist[g, :, c, :], (np.broadcast_to(tt[None, :], k[:, c].shape)[w], k[:, c][w]), 1)
    return hist


def _prob(B=64, T=10):
    p = _lib.Problem()
    p.B, p.T = B, T
    p.RRt[:] = [1e-5, 0.0, 0.0, 1e-5]
    return p


def test_abi_revision_and_symbols():
    _lib.build_library()
    lib = _lib.lib()
    assert lib.aoc_abi_version() == _lib.AOC_ABI_VERSION == 5
    assert _lib.AOC_HIST_NCH == NCH and _lib.AOC_HIST_NBIN == NBIN
    for name in ("aoc_track_ensemble_histogram", "aoc_ensemble_histogram_scratch_bytes"):
        assert name in _lib.SYMBOLS and getattr(lib, name)
    hdr = open(_lib._HDR).read()
    assert "#define AOC_HIST_NCH  8" in hdr and "#define AOC_HIST_NBIN 64" in hdr and "#define AOC_ABI_VERSION 5" in hdr
    assert len(_lib.SYMBOLS["aoc_track_ensemble_histogram"][1]) == 15
    # the older entry points keep their argument lists
    assert len(_lib.SYMBOLS["aoc_track_ensemble"][1]) == 11 and len(_lib.SYMBOLS["aoc_track_ensemble_envelope"][1]) == 14


def test_scratch_query():
    """one byte per tile, sample, channel and bin; geometry the call would refuse asks for nothing"""
    q = _lib.lib().aoc_ensemble_histogram_scratch_bytes
    assert q(64, 10, 64) == 1 * 10 * NCH * NBIN
    assert q(322, 1000, 192) == 6 * 1000 * NCH * NBIN
    assert q(65536, 1000, 65536) == 1024 * 1000 * NCH * NBIN
    assert q(0, 10, 64) == 0 and q(64, 10, 100) == 0 and q(64, 0, 64) == 0


def test_argument_errors_carry_a_reason():
    lib = _lib.lib()
    big = 1 << 40

    def call(p, n_opt=1, mpo=64, nominal=16, x0=16, noise=None, bins=16, x=None, u=None, dist=None, stats=16, status=None,
             hist=16, scratch=16, scratch_bytes=big):
        return lib.aoc_track_ensemble_histogram(C.byref(p) if p is not None else None, n_opt, mpo, nominal, x0, noise, bins, x,
                                                u, dist, stats, status, hist, scratch, scratch_bytes)
    nz = C.byref(_lib.MpcNoise(1, 0, 0, (C.c_double * 6)(*[1e-3] * 6)))
    f32 = _prob()
    f32.x_out_f32 = 1
    rsym = _prob()
    rsym.RRt[1] = 1e-7
    need = lib.aoc_ensemble_histogram_scratch_bytes(64, 10, 64)
    assert need > 0
    cases = [
        # the new arguments
        (dict(p=_prob(), bins=None), b"bins is NULL"),
        (dict(p=_prob(), hist=None), b"hist is NULL"),
        (dict(p=_prob(), scratch_bytes=need - 1), b"scratch_bytes = %d, need %d" % (need - 1, need)),
        (dict(p=_prob(), scratch_bytes=0), b"scratch_bytes = 0"),
        (dict(p=_prob(), scratch=None), b"scratch is NULL"),
        (dict(p=_prob(), scratch=8), b"16-byte aligned"),
        (dict(p=_prob(), hist=4), b"16-byte aligned"),
        # every case of tests/test_ensemble_abi.py::test_argument_errors_carry_a_reason
        (dict(p=None), b"aoc_problem is NULL"),
        (dict(p=_prob(), nominal=None), b"nominal is NULL"),
        (dict(p=_prob(), x0=None), b"x0_reg is NULL"),
        (dict(p=_prob(), stats=None), b"stats is NULL"),
        (dict(p=_prob(), n_opt=0), b"n_opt = 0"),
        (dict(p=_prob(), mpo=0), b"members_per_opt = 0"),
        (dict(p=_prob(), mpo=100), b"members_per_opt = 100"),
        (dict(p=_prob(), mpo=-64), b"members_per_opt = -64"),
        (dict(p=_prob(T=2)), b"T = 2"),
        (dict(p=_prob(B=65)), b"B = 65"),                          # more members than n_opt * members_per_opt
        (dict(p=_prob(B=128), n_opt=3), b"B = 128"),               # the last group would be empty
        (dict(p=_prob(B=0)), b"B = 0"),
        (dict(p=_prob(), x=16), b"x_reg and u_reg go together"),
        (dict(p=_prob(), u=16), b"x_reg and u_reg go together"),
        (dict(p=f32, x=16, u=16, noise=nz), b"float32"),
        (dict(p=rsym), b"RRt is not symmetric"),
    ]
    for kw, reason in cases:
        # leave another reason behind first, so that an error return without a new reason shows
        q = _lib.Problem()
        q.B, q.T, q.ref = 4, 2, 1
        assert lib.aoc_traj_cost(C.byref(q), 1, 1, 1, 1) == -1 and b"T = 2 " in lib.aoc_last_hip_error() + b" "
        assert call(**kw) == -1, kw
        msg = lib.aoc_last_hip_error()
        assert msg.startswith(b"aoc_track_ensemble_histogram: ") and reason in msg, (kw, msg)
    # and the older entry points still name themselves
    assert lib.aoc_track_ensemble(C.byref(_prob()), 1, 64, None, 1, None, None, None, None, 1, None) == -1
    assert lib.aoc_last_hip_error().startswith(b"aoc_track_ensemble: nominal is NULL")
    assert lib.aoc_track_ensemble_envelope(C.byref(_prob()), 1, 64, 1, 1, None, None, None, None, 1, None, None, 1, big) == -1
    assert lib.aoc_last_hip_error().startswith(b"aoc_track_ensemble_envelope: envelope is NULL")


def test_histogram_bins_on_hand_made_records():
    from aircraftoptimalcontrol_amd import batch
    raw = np.zeros((2, 3, 44))
    raw[..., 1:7], raw[..., 13:15] = np.inf, np.inf          # the empty set everywhere first
    raw[..., 7:13], raw[..., 15:17] = -np.inf, -np.inf
    # optimum 0, sample 0: the ordinary case, channel by channel
    mn = np.array([-1.0, 0.0, 2.0, -8.0, 0.5, -0.25, -3.0, 1.0])
    mx = np.array([1.0, 4.0, 2.5, -4.0, 64.5, 0.25, 5.0, 1.5])
    raw[0, 0, 0] = 10
    raw[0, 0, 1:7], raw[0, 0, 7:13], raw[0, 0, 13:15], raw[0, 0, 15:17] = mn[:6], mx[:6], mn[6:], mx[6:]
    # optimum 0, sample 1: max == min (one member, or all on one value): channel 2 at 0.75
    raw[0, 1, 0] = 1
    raw[0, 1, 1:7], raw[0, 1, 7:13] = 0.75, 0.75
    raw[0, 1, 13:15], raw[0, 1, 15:17] = -0.5, -0.5
    # everything else: n = 0
    b = batch.histogram_bins(raw)
    assert b.shape == (2, 3, NCH, 2) and b.dtype == np.float64 and np.isfinite(b).all()
    assert np.array_equal(b[0, 0, :, 0], mn) and np.array_equal(b[0, 0, :, 1], 64.0 / (mx - mn))
    assert np.array_equal(b[0, 1, :6], np.tile([0.75, 0.0], (6, 1))) and np.array_equal(b[0, 1, 6:], np.tile([-0.5, 0.0], (2, 1)))
    assert not b[0, 2].any() and not b[1].any()
    # (T,44) is one optimum
    assert np.array_equal(batch.histogram_bins(raw[0]), b[:1])
    # pad widens the range on either side by its share of max - min
    p = batch.histogram_bins(raw, pad=0.25)
    assert np.array_equal(p[0, 0, :, 0], mn - 0.25 * (mx - mn)) and np.array_equal(p[0, 0, :, 1], 64.0 / ((mx - mn) * 1.5))
    assert np.array_equal(p[0, 1:], b[0, 1:]) and np.array_equal(p[1], b[1])
    # the largest value lands in bin 63, the smallest in bin 0, under the device's rule
    for v, k in ((mx, 63), (mn, 0)):
        s = (v - b[0, 0, :, 0]) * b[0, 0, :, 1]
        assert np.array_equal(np.where(s >= 63, 63, np.where(s >= 1, s.astype(int), 0)), np.full(NCH, k))
    with pytest.raises(ValueError):
        batch.histogram_bins(np.zeros((3, 43)))


def _skewed_ensemble(seed=11, M=200, T=50):
    """M members about one nominal, skewed (log-normal about the nominal); members 3, 77 and 150 leave mid-way (first_bad
    set by hand, their samples from there on NaN), member 199 never counts."""
    rng = np.random.default_rng(seed)
    xo, uo = rng.normal(size=(6, T)), rng.normal(size=(2, T))
    xx = xo + (np.exp(rng.normal(size=(M, 6, T)) * 0.8) - 0.5) * np.array([0.3, 0.3, 0.5, 0.05, 0.1, 0.05])[None, :, None]
    uu = uo - np.exp(rng.normal(size=(M, 2, T))) * 0.1
    fb = np.full(M, T)
    for b, t in ((3, 10), (77, 25), (150, 49), (199, 0)):
        fb[b] = t
        xx[b, :, t:], uu[b, :, t:] = np.nan, np.nan
    return xx, uu, xo, uo, fb


def _minmax_records(xx, uu, xo, uo, fb):
    """what histogram_bins reads of an envelope record (n, min, max), from the trajectories of ONE optimum"""
    M, T = xx.shape[0], xx.shape[2]
    c3 = (np.arange(T)[None, :] < fb[:, None])[:, None, :]
    v = np.concatenate([xx - xo, uu - uo], axis=1)
    raw = np.zeros((1, T, 44))
    raw[0, :, 0] = c3[:, 0].sum(axis=0)
    lo, hi = np.where(c3, v, np.inf).min(axis=0).T, np.where(c3, v, -np.inf).max(axis=0).T      # (T,8)
    lo[T - 1, 6:], hi[T - 1, 6:] = np.inf, -np.inf
    raw[0, :, 1:7], raw[0, :, 13:15], raw[0, :, 7:13], raw[0, :, 15:17] = lo[:, :6], lo[:, 6:], hi[:, :6], hi[:, 6:]
    return raw


def test_merge_of_two_halves_is_the_whole():
    from aircraftoptimalcontrol_amd import batch
    xx, uu, xo, uo, fb = _skewed_ensemble()
    M, T = xx.shape[0], xx.shape[2]
    bins = batch.histogram_bins(_minmax_records(xx, uu, xo, uo, fb))
    whole = numpy_histogram(xx, uu, xo, uo, fb, np.zeros(M, int), bins)
    h = M // 2
    a = numpy_histogram(xx[:h], uu[:h], xo, uo, fb[:h], np.zeros(h, int), bins)
    b = numpy_histogram(xx[h:], uu[h:], xo, uo, fb[h:], np.zeros(M - h, int), bins)
    m = batch.histogram_merge(a.astype(np.int32), b.astype(np.int32))
    assert m.shape == whole.shape == (1, T, NCH, NBIN) and m.dtype.kind == "i" and np.array_equal(m, whole)
    n = (np.arange(T)[:, None] < fb[None, :]).sum(axis=1)
    assert np.array_equal(whole[0, :, :6].sum(axis=-1), np.repeat(n[:, None], 6, 1)) and n[0] == M - 1 and n[-1] == M - 4
    assert np.array_equal(whole[0, :T - 1, 6:].sum(axis=-1), np.repeat(n[:T - 1, None], 2, 1)) and not whole[0, T - 1, 6:].any()
    with pytest.raises(ValueError):
        batch.histogram_merge(a, b[:, :-1])
    with pytest.raises(ValueError):
        batch.histogram_merge(a, b.astype(np.float64))


def test_quantiles_against_order_statistics():
    """200 members, T = 50, skewed values, members dropping out mid-way: for every q, sample and channel the tube is within
    one bin width of the r-th order statistic of the members that count (module docstring)."""
    from aircraftoptimalcontrol_amd import batch
    xx, uu, xo, uo, fb = _skewed_ensemble()
    M, T = xx.shape[0], xx.shape[2]
    bins = batch.histogram_bins(_minmax_records(xx, uu, xo, uo, fb))
    hist = numpy_histogram(xx, uu, xo, uo, fb, np.zeros(M, int), bins)
    qs = (0.0, 0.01, 0.05, 0.25, 0.5, 0.9, 0.95, 0.99, 1.0)
    tube, width = batch.histogram_quantiles(hist, bins, qs)
    assert tube.shape == (len(qs), 1, NCH, T) and width.shape == (1, NCH, T)
    v = np.concatenate([xx - xo, uu - uo], axis=1)
    worst = 0.0
    for t in range(T):
        live = np.flatnonzero(fb > t)
        for c in range(NCH):
            if c >= 6 and t == T - 1:
                assert np.isnan(tube[:, 0, c, t]).all() and width[0, c, t] == 0.0       # n = 0
                continue
            srt = np.sort(v[live, c, t])
            assert width[0, c, t] == 1.0 / bins[0, t, c, 1] > 0
            for i, f in enumerate(qs):
                r = max(1, int(np.ceil(f * live.size)))
                err = abs(tube[i, 0, c, t] - srt[r - 1])
                worst = max(worst, err / width[0, c, t])
                assert err <= width[0, c, t], (f, t, c, err, width[0, c, t])
    print("largest |tube - order statistic| / width = %.3f" % worst)
    # (T,8,64) with (T,8,2) is one optimum; inv_w = 0 gives lo; the levels are checked
    t1, w1 = batch.histogram_quantiles(hist[0], bins[0], [0.5])
    assert np.array_equal(t1, tube[4:5], equal_nan=True) and np.array_equal(w1, width)
    one = np.zeros((1, 1, NCH, NBIN), dtype=np.int32)
    one[..., 0] = 7
    b0 = np.zeros((1, 1, NCH, 2))
    b0[..., 0] = 0.75
    t0, w0 = batch.histogram_quantiles(one, b0, (0.05, 0.95))
    assert (t0 == 0.75).all() and not w0.any()
    with pytest.raises(ValueError):
        batch.histogram_quantiles(hist, bins, [1.5])
    with pytest.raises(ValueError):
        batch.histogram_quantiles(hist, bins[:, :-1], [0.5])
